"""Scores of a predictive ensemble against data: lppd, WAIC, PIT coverage and the CRPS.

One device call (`qn_pred_score`, csrc/qn_score.hip) reduces the `(M, K)` member predictions -- member m predicts
N(f_mk, noise^2 + V_mk) for entry k, the predictive is the equal-weight mixture -- to six numbers per entry; `summarise`
turns that `[6, K]` array into the scalar scores on the host.  On training data `waic` is the WAIC (Gelman, Hwang &
Vehtari, Stat. Comput. 24, 2014, p_waic2); on held-out data `nlpd` is the test negative log predictive density.  The CRPS
of a Gaussian mixture is the closed form of Grimit et al. (Q. J. R. Meteorol. Soc. 132, 2006); its pair term costs
O(M^2 K) evaluations.  With loo=True a second device call (`qn_psis_loo`, csrc/qn_psis.hip) adds the Pareto-smoothed
importance-sampling leave-one-out scores: `elpd_loo`, the per-entry `khat` that says where it can be trusted, and the LOO-PIT
(`psis.py` is their contract in numpy).  `group_lpd`, `stack_weights` and `member_weights=` are the stacking of groups of
members -- chains that did not mix, deep-ensemble members -- on the device (`qn_group_lpd`, `qn_stack_weights`,
`qn_pred_score_w`, csrc/qn_stack.hip; `stacking.py` is their contract, include/quinn_amd_stack.h their header).  `quantile_rows`,
`pred_quantiles` and `interval_summary` are the inverse of the PIT: the quantiles and credible bands of the same mixture
(`qn_pred_quantile`, csrc/qn_quantile.hip; `predquant.py` is the contract, include/quinn_amd_quantile.h the header).  Rank histograms and energy scores across outputs are out of scope.  The reference
has no counterpart; the per-entry definitions are in include/quinn_amd.h at `qn_pred_score` and in include/quinn_amd_psis.h at `qn_psis_loo`.
"""

import numpy as np
import torch

from . import _lib
from .psis import khat_threshold, summarise_loo  # noqa: F401  (re-exported)
from .stacking import DEFAULT_MAX_ITER, DEFAULT_TOL

ROWS = ("lppd_k", "p_waic_k", "pit", "crps_k", "mean", "var")          # the rows of qn_pred_score's output, in order
DEFAULT_LEVELS = (0.5, 0.9, 0.95)
WHAT_ALL = _lib.SCORE_LPPD | _lib.SCORE_PWAIC | _lib.SCORE_PIT | _lib.SCORE_CRPS | _lib.SCORE_MOMENTS


def summarise(rows, y, levels=DEFAULT_LEVELS):
    """The score dict from the `[6, K]` per-entry rows (numpy; a row that was not computed is NaN) and the targets `y`
    (K values in any shape; the per-entry arrays come back in that shape).

    Per entry: `lppd_k`, `p_waic_k`, `pit`, `crps_k`, `mean`, `var`.  Scalars: `lppd` = sum lppd_k, `p_waic` = sum p_waic_k,
    `elpd_waic` = lppd - p_waic, `waic` = -2 elpd_waic, `se_elpd` = sqrt(K var_k(lppd_k - p_waic_k)) (ddof = 1; NaN for
    K = 1), `nlpd` = -lppd / K, `crps` = mean crps_k, `rmse` of `mean` against y, `coverage[level]` = the share of entries
    whose PIT lies in the central interval of that level, |pit - 0.5| <= level / 2, and `pit_hist`, the counts of 10 equal
    bins of [0, 1].  `n` = K."""
    y = np.asarray(y, dtype=np.float64)
    rows = np.asarray(rows, dtype=np.float64)
    K = y.size
    if rows.shape != (_lib.SCORE_NOUT, K) or K < 1:
        raise ValueError(f"rows of shape {rows.shape}; expected ({_lib.SCORE_NOUT}, {K}) for y of shape {y.shape}")
    res = {name: rows[i].reshape(y.shape).copy() for i, name in enumerate(ROWS)}
    lppd_k, p_k, pit, crps_k, mean = rows[0], rows[1], rows[2], rows[3], rows[4]
    elpd_k = lppd_k - p_k
    res["n"] = K
    res["lppd"] = float(lppd_k.sum())
    res["p_waic"] = float(p_k.sum())
    res["elpd_waic"] = res["lppd"] - res["p_waic"]
    res["waic"] = -2.0 * res["elpd_waic"]
    res["se_elpd"] = float(np.sqrt(K * elpd_k.var(ddof=1))) if K > 1 else float("nan")
    res["nlpd"] = -res["lppd"] / K
    res["crps"] = float(crps_k.mean())
    res["rmse"] = float(np.sqrt(np.mean((mean - y.reshape(-1)) ** 2)))
    res["coverage"] = {float(lv): float(np.mean(np.abs(pit - 0.5) <= 0.5 * float(lv))) for lv in levels}
    res["pit_hist"] = np.histogram(pit[np.isfinite(pit)], bins=10, range=(0.0, 1.0))[0]
    return res


def score_rows(F, y, noise, V=None, what=WHAT_ALL):
    """`qn_pred_score` on device tensors: F `(M, K)` float64 / float32 contiguous, V the same or None, y `(K,)` float64
    -> `[6, K]` float64 device tensor; rows `what` does not ask for are NaN."""
    M, K = F.shape
    L = _lib.lib()
    need = int(L.qn_pred_score_workspace_bytes(M, K, what))
    if need == 0:
        raise ValueError(L.qn_last_error().decode())
    if V is not None and (V.shape != F.shape or V.dtype != F.dtype or V.device != F.device):
        raise ValueError("V must match F in shape, dtype and device")
    if y.shape != (K,) or y.dtype != torch.float64 or y.device != F.device:
        raise ValueError(f"y: a float64 tensor of {K} entries on F's device is needed")
    out = torch.full((_lib.SCORE_NOUT, K), float("nan"), dtype=torch.float64, device=F.device)
    ws = torch.empty(need // 8, dtype=torch.float64, device=F.device)
    qdt = _lib.QN_F32 if F.dtype == torch.float32 else _lib.QN_F64
    with torch.cuda.device(F.device):
        st = _lib.stream(F.device)
        _lib.check(L.qn_pred_score(F.data_ptr(), V.data_ptr() if V is not None else None, qdt, y.data_ptr(), M, K,
                                   float(noise), what, out.data_ptr(), ws.data_ptr(), need, st), "qn_pred_score")
    return out


def psis_rows(F, y, noise, V=None):
    """`qn_psis_loo` on device tensors: F `(M, K)` float64 / float32 contiguous, V the same or None, y `(K,)` float64
    -> `[4, K]` float64 device tensor (elpd_loo_k, khat, ess_k, pit_loo)."""
    M, K = F.shape
    L = _lib.lib()
    need = int(L.qn_psis_loo_workspace_bytes(M, K))
    if need == 0:
        raise ValueError(L.qn_last_error().decode())
    if V is not None and (V.shape != F.shape or V.dtype != F.dtype or V.device != F.device):
        raise ValueError("V must match F in shape, dtype and device")
    if y.shape != (K,) or y.dtype != torch.float64 or y.device != F.device:
        raise ValueError(f"y: a float64 tensor of {K} entries on F's device is needed")
    out = torch.empty((_lib.LOO_NOUT, K), dtype=torch.float64, device=F.device)
    ws = torch.empty(need // 8, dtype=torch.float64, device=F.device)
    qdt = _lib.QN_F32 if F.dtype == torch.float32 else _lib.QN_F64
    with torch.cuda.device(F.device):
        st = _lib.stream(F.device)
        _lib.check(L.qn_psis_loo(F.data_ptr(), V.data_ptr() if V is not None else None, qdt, y.data_ptr(), M, K,
                                 float(noise), out.data_ptr(), ws.data_ptr(), need, st), "qn_psis_loo")
    return out


def _check_fvy(F, V, y):
    K = F.shape[1]
    if V is not None and (V.shape != F.shape or V.dtype != F.dtype or V.device != F.device):
        raise ValueError("V must match F in shape, dtype and device")
    if y is not None and (y.shape != (K,) or y.dtype != torch.float64 or y.device != F.device):
        raise ValueError(f"y: a float64 tensor of {K} entries on F's device is needed")


def score_rows_w(F, y, noise, wm, V=None, what=WHAT_ALL):
    """`qn_pred_score_w` on device tensors: `score_rows` for the mixture with the member weights wm `(M,)` (float64 device
    tensor, >= 0, sum 1; a member of weight 0 is skipped, a negative or non-finite weight makes every row NaN).  y may be
    None when `what` is SCORE_MOMENTS."""
    M, K = F.shape
    L = _lib.lib()
    need = int(L.qn_pred_score_w_workspace_bytes(M, K, what))
    if need == 0:
        raise ValueError(L.qn_last_error().decode())
    _check_fvy(F, V, y)
    if wm.shape != (M,) or wm.dtype != torch.float64 or wm.device != F.device:
        raise ValueError(f"member_weights: a float64 tensor of {M} weights on F's device is needed")
    out = torch.full((_lib.SCORE_NOUT, K), float("nan"), dtype=torch.float64, device=F.device)
    ws = torch.empty(need // 8, dtype=torch.float64, device=F.device)
    qdt = _lib.QN_F32 if F.dtype == torch.float32 else _lib.QN_F64
    with torch.cuda.device(F.device):
        st = _lib.stream(F.device)
        _lib.check(L.qn_pred_score_w(F.data_ptr(), V.data_ptr() if V is not None else None, qdt,
                                     y.data_ptr() if y is not None else None, wm.data_ptr(), M, K, float(noise), what,
                                     out.data_ptr(), ws.data_ptr(), need, st), "qn_pred_score_w")
    return out


def group_lpd_rows(F, y, noise, offsets, V=None):
    """`qn_group_lpd` on device tensors: L `[G, K]` float64 device tensor, L_gk the log density of entry k under the members
    offsets[g] .. offsets[g + 1] - 1 of F `(M, K)` alone."""
    M, K = F.shape
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    G = len(offsets) - 1
    L = _lib.lib()
    need = int(L.qn_group_lpd_workspace_bytes(M, K, G))
    if need == 0:
        raise ValueError(L.qn_last_error().decode())
    _check_fvy(F, V, y)
    out = torch.empty((G, K), dtype=torch.float64, device=F.device)
    ws = torch.empty(need // 8, dtype=torch.float64, device=F.device)
    qdt = _lib.QN_F32 if F.dtype == torch.float32 else _lib.QN_F64
    with torch.cuda.device(F.device):
        st = _lib.stream(F.device)
        _lib.check(L.qn_group_lpd(F.data_ptr(), V.data_ptr() if V is not None else None, qdt, y.data_ptr(), M, K, float(noise),
                                  offsets.ctypes.data, G, out.data_ptr(), ws.data_ptr(), need, st), "qn_group_lpd")
    return out


def group_lpd(F, y, noise, offsets, V=None, loo=False):
    """(L `[G, K]` float64 device tensor, khat_bad_share `[G]` or None): the log predictive density of every entry under each
    group of members alone, groups offsets[g] .. offsets[g + 1] - 1 of F `(M, K)` (device tensors as in `score_rows`).
    loo=False: `qn_group_lpd`, one pass, for held-out y.  loo=True, for the data the members were fitted to: row 0 of
    `psis_rows` on every group's slice (groups of at least 2 members), and each group's share of entries whose khat lies above
    `khat_threshold(M_g)` -- where its leave-one-out density is not to be trusted."""
    if not loo:
        return group_lpd_rows(F, y, noise, offsets, V), None
    offsets = np.asarray(offsets, dtype=np.int64)
    G = len(offsets) - 1
    if offsets[0] != 0 or offsets[-1] != F.shape[0] or np.any(np.diff(offsets) < 2):
        raise ValueError("loo=True needs groups of at least 2 members, offsets rising from 0 to M")
    out = torch.empty((G, F.shape[1]), dtype=torch.float64, device=F.device)
    share = torch.empty(G, dtype=torch.float64, device=F.device)
    for g in range(G):
        lo, hi = int(offsets[g]), int(offsets[g + 1])
        rows = psis_rows(F[lo:hi], y, noise, None if V is None else V[lo:hi])
        out[g] = rows[0]
        share[g] = (rows[1] > khat_threshold(hi - lo)).double().mean()
    return out, share.cpu().numpy()


def stack_weights(L, tol=DEFAULT_TOL, max_iter=DEFAULT_MAX_ITER, block=64):
    """`qn_stack_weights`: the stacking weights of L `[G, K]` (float64 device tensor; -Inf is density 0), the dict of
    `stacking.stack_weights` with `w` a numpy array.  The EM launches are enqueued in blocks of `block`; the status of a block
    is looked at after the next one has been enqueued, and launches after the stopping iterate are no-ops on a device flag,
    so neither `w` nor `iters` depends on `block`."""
    if L.dim() != 2 or L.dtype != torch.float64 or not L.is_cuda or not L.is_contiguous():
        raise ValueError("L: a contiguous float64 device tensor [G, K] is needed")
    G, K = L.shape
    lib = _lib.lib()
    need = int(lib.qn_stack_weights_workspace_bytes(G, K))
    if need == 0:
        raise ValueError(lib.qn_last_error().decode())
    block, max_iter = int(block), int(max_iter)
    if block < 1:
        raise ValueError("block >= 1 is needed")
    dev = L.device
    w = torch.empty(G, dtype=torch.float64, device=dev)
    status = torch.empty(_lib.STACK_NSTATUS, dtype=torch.float64, device=dev)
    ws = torch.empty(need // 8, dtype=torch.float64, device=dev)
    pending = []                                                 # (pinned snapshot of the status, event), oldest first
    t, final = 0, None
    with torch.cuda.device(dev):
        st = _lib.stream(dev)
        while final is None:
            if t < max_iter + 2:
                n = min(block, max_iter + 2 - t)
                _lib.check(lib.qn_stack_weights(L.data_ptr(), G, K, float(tol), max_iter, t, n, w.data_ptr(), status.data_ptr(),
                                                ws.data_ptr(), need, st), "qn_stack_weights")
                t += n
                snap = torch.empty(_lib.STACK_NSTATUS, dtype=torch.float64).pin_memory()
                snap.copy_(status, non_blocking=True)
                ev = torch.cuda.Event()
                ev.record()
                pending.append((snap, ev))
            if len(pending) > 1 or t >= max_iter + 2:
                snap, ev = pending.pop(0)
                ev.synchronize()
                if snap[-1] != 0:
                    final = snap
                elif not pending and t >= max_iter + 2:
                    raise _lib.QuinnAmdError("qn_stack_weights: no iterate stopped within max_iter + 2 launches")
        wh = w.cpu().numpy()
    s = final.numpy()
    return {"w": wh, "obj": float(s[0]), "gap": float(s[1]), "iters": int(s[2]), "n_kept": int(s[3]), "n_nonfinite": int(s[4]),
            "n_dropped": int(s[5]), "obj_equal": float(s[6])}


def quantile_rows(F, q, noise, V=None, wm=None, return_iters=False):
    """`qn_pred_quantile` on device tensors: F `(M, K)` float64 / float32 contiguous, V the same or None, wm `(M,)` float64
    member weights or None (1 / M), q the levels (host values) -> `[Q, K]` float64 device tensor of the quantiles of the
    mixture sum_m wm_m N(f_mk, noise^2 + V_mk).  noise == 0 without V: the order-statistic quantiles of the members, levels
    in [0, 1]; otherwise the roots of the mixture's distribution function, levels in (0, 1).  return_iters: also the `(K,)`
    int32 device tensor of the largest number of evaluations an entry's levels took (0 in the order-statistic mode)."""
    M, K = F.shape
    q = np.ascontiguousarray(np.asarray(q, dtype=np.float64).reshape(-1))
    Q = q.size
    L = _lib.lib()
    need = int(L.qn_pred_quantile_workspace_bytes(M, K, Q, int(float(noise) == 0.0 and V is None)))
    if need == 0:
        raise ValueError(L.qn_last_error().decode())
    _check_fvy(F, V, None)
    if wm is not None and (wm.shape != (M,) or wm.dtype != torch.float64 or wm.device != F.device):
        raise ValueError(f"member_weights: a float64 tensor of {M} weights on F's device is needed")
    out = torch.empty((Q, K), dtype=torch.float64, device=F.device)
    iters = torch.empty(K, dtype=torch.int32, device=F.device) if return_iters else None
    ws = torch.empty(need // 8, dtype=torch.float64, device=F.device)
    qdt = _lib.QN_F32 if F.dtype == torch.float32 else _lib.QN_F64
    with torch.cuda.device(F.device):
        st = _lib.stream(F.device)
        rc = L.qn_pred_quantile(F.data_ptr(), V.data_ptr() if V is not None else None, qdt,
                                wm.data_ptr() if wm is not None else None, M, K, float(noise), q.ctypes.data, Q, out.data_ptr(),
                                iters.data_ptr() if iters is not None else None, ws.data_ptr(), need, st)
    if rc == _lib.CONSTANTS["QN_EINVAL"]:
        raise ValueError(L.qn_last_error().decode())
    _lib.check(rc, "qn_pred_quantile")
    return (out, iters) if return_iters else out


def pred_quantiles(F, q, noise, V=None, member_weights=None, device=None):
    """The quantiles at the levels q of the predictive of the ensemble F `(M, N, o)` or `(M, K)` (device tensor or numpy;
    float32 is read as it is, all arithmetic is float64): member m predicts N(F[m], noise^2 + V[m]), mixed with the weights
    member_weights `(M,)` (>= 0, sum 1; None: equal).  Returns numpy `(Q,) + F.shape[1:]`.  noise = 0 without V gives the
    order-statistic quantiles of the members (np.quantile's default method with equal weights).  Only the `Q x K` result
    leaves the device."""
    if isinstance(F, torch.Tensor) and F.is_cuda:
        dev = F.device
    else:
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    shape = tuple(F.shape[1:])
    K = int(np.prod(shape))
    Ft = _ens_tensor(F, K, dev, "F")
    Vt = None if V is None else _ens_tensor(V, K, dev, "V").to(Ft.dtype)
    wm = None if member_weights is None else torch.as_tensor(np.asarray(member_weights, dtype=np.float64).reshape(-1), device=dev)
    rows = quantile_rows(Ft, q, noise, Vt, wm).cpu().numpy()
    return rows.reshape((rows.shape[0],) + shape)


def interval_summary(qlo, qhi, y, level):
    """The width, coverage and interval score of the central `level` band [qlo, qhi] against the targets y (numpy, any common
    shape): `width` = mean(qhi - qlo), `coverage` = the share of y inside the closed band, `interval_score` = the mean
    Winkler score, width + (2 / (1 - level)) (distance of y outside the band) (Gneiting & Raftery, JASA 102, 2007), and `n`."""
    qlo, qhi, y = (np.asarray(a, dtype=np.float64) for a in (qlo, qhi, y))
    if not (qlo.shape == qhi.shape == y.shape) or y.size < 1 or not 0.0 < float(level) < 1.0:
        raise ValueError(f"qlo {qlo.shape}, qhi {qhi.shape} and y {y.shape} must share a shape, and 0 < level < 1")
    width = qhi - qlo
    outside = np.maximum(qlo - y, 0.0) + np.maximum(y - qhi, 0.0)
    return {"n": int(y.size), "level": float(level), "width": float(width.mean()),
            "coverage": float(np.mean((y >= qlo) & (y <= qhi))),
            "interval_score": float(np.mean(width + (2.0 / (1.0 - float(level))) * outside))}


def summarise_all(rows, loo_rows, y, M, levels=DEFAULT_LEVELS):
    """`summarise(rows, y)`, and with `loo_rows` (the `[4, K]` rows of `qn_psis_loo`, or None) the keys of `summarise_loo`
    and `p_loo` = lppd - elpd_loo beside them."""
    res = summarise(rows, y, levels)
    if loo_rows is not None:
        res.update(summarise_loo(loo_rows, y, M, lppd=res["lppd"], levels=levels))
    return res


def _ens_tensor(a, K, device, name):
    """`(M, K)` contiguous float64 / float32 device tensor of an `(M, N, o)` or `(M, K)` ensemble array."""
    t = a if isinstance(a, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(a))
    if t.dtype not in (torch.float32, torch.float64):
        t = t.double()
    if t.dim() < 2 or t[0].numel() != K:
        raise ValueError(f"{name} of shape {tuple(t.shape)} does not hold {K} entries per member")
    return t.to(device).reshape(t.shape[0], K).contiguous()


def pred_score(F, y, noise, V=None, crps=True, levels=DEFAULT_LEVELS, device=None, loo=False, member_weights=None):
    """Score the predictive ensemble F `(M, N, o)` or `(M, K)` (device tensor or numpy; float32 is read as it is, all
    arithmetic is float64) against the targets y `(N, o)` / `(K,)`: member m predicts N(F[m], noise^2 + V[m]), V an optional
    per-member predictive variance shaped like F.  Returns the dict of `summarise`.  crps=False skips the O(M^2 K) pair pass
    (`crps_k` and `crps` are NaN).  loo=True adds the PSIS-LOO keys of `summarise_loo` and `p_loo` (one more device call).
    Only the `6 x K` (with loo, `10 x K`) result leaves the device.  member_weights `(M,)` (>= 0, sum 1; e.g. from stacking)
    scores the weighted mixture instead of the equal-weight one (`qn_pred_score_w`; not together with loo)."""
    if member_weights is not None and loo:
        raise ValueError("loo=True scores the equal-weight ensemble: not together with member_weights")
    y = np.asarray(y, dtype=np.float64)
    if isinstance(F, torch.Tensor) and F.is_cuda:
        dev = F.device
    else:
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    Ft = _ens_tensor(F, y.size, dev, "F")
    Vt = None if V is None else _ens_tensor(V, y.size, dev, "V").to(Ft.dtype)
    what = WHAT_ALL if crps else WHAT_ALL & ~_lib.SCORE_CRPS
    yt = torch.as_tensor(y.reshape(-1), device=dev)
    if member_weights is not None:
        wm = torch.as_tensor(np.asarray(member_weights, dtype=np.float64).reshape(-1), device=dev)
        return summarise(score_rows_w(Ft, yt, noise, wm, Vt, what).cpu().numpy(), y, levels)
    loo_rows = psis_rows(Ft, yt, noise, Vt).cpu().numpy() if loo else None
    return summarise_all(score_rows(Ft, yt, noise, Vt, what).cpu().numpy(), loo_rows, y, Ft.shape[0], levels)
