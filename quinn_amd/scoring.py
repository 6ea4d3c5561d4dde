"""Scores of a predictive ensemble against data: lppd, WAIC, PIT coverage and the CRPS.

One device call (`qn_pred_score`, csrc/qn_score.hip) reduces the `(M, K)` member predictions -- member m predicts
N(f_mk, noise^2 + V_mk) for entry k, the predictive is the equal-weight mixture -- to six numbers per entry; `summarise`
turns that `[6, K]` array into the scalar scores on the host.  On training data `waic` is the WAIC (Gelman, Hwang &
Vehtari, Stat. Comput. 24, 2014, p_waic2); on held-out data `nlpd` is the test negative log predictive density.  The CRPS
of a Gaussian mixture is the closed form of Grimit et al. (Q. J. R. Meteorol. Soc. 132, 2006); its pair term costs
O(M^2 K) evaluations.  With loo=True a second device call (`qn_psis_loo`, csrc/qn_psis.hip) adds the Pareto-smoothed
importance-sampling leave-one-out scores: `elpd_loo`, the per-entry `khat` that says where it can be trusted, and the LOO-PIT
(`psis.py` is their contract in numpy).  Rank histograms and energy scores across outputs are out of scope.  The reference
has no counterpart; the per-entry definitions are in include/quinn_amd.h at `qn_pred_score` and in include/quinn_amd_psis.h at `qn_psis_loo`.
"""

import numpy as np
import torch

from . import _lib
from .psis import summarise_loo  # noqa: F401  (re-exported)

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


def pred_score(F, y, noise, V=None, crps=True, levels=DEFAULT_LEVELS, device=None, loo=False):
    """Score the predictive ensemble F `(M, N, o)` or `(M, K)` (device tensor or numpy; float32 is read as it is, all
    arithmetic is float64) against the targets y `(N, o)` / `(K,)`: member m predicts N(F[m], noise^2 + V[m]), V an optional
    per-member predictive variance shaped like F.  Returns the dict of `summarise`.  crps=False skips the O(M^2 K) pair pass
    (`crps_k` and `crps` are NaN).  loo=True adds the PSIS-LOO keys of `summarise_loo` and `p_loo` (one more device call).
    Only the `6 x K` (with loo, `10 x K`) result leaves the device."""
    y = np.asarray(y, dtype=np.float64)
    if isinstance(F, torch.Tensor) and F.is_cuda:
        dev = F.device
    else:
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    Ft = _ens_tensor(F, y.size, dev, "F")
    Vt = None if V is None else _ens_tensor(V, y.size, dev, "V").to(Ft.dtype)
    what = WHAT_ALL if crps else WHAT_ALL & ~_lib.SCORE_CRPS
    yt = torch.as_tensor(y.reshape(-1), device=dev)
    loo_rows = psis_rows(Ft, yt, noise, Vt).cpu().numpy() if loo else None
    return summarise_all(score_rows(Ft, yt, noise, Vt, what).cpu().numpy(), loo_rows, y, Ft.shape[0], levels)
