"""Convergence diagnostics of many chains: split-R-hat, batch-means ESS and pooled moments.

One streaming device pass (`qn_chain_stats`, csrc/qn_diag.hip) reduces a `[C, T, K]` stack of chains to `[C, 6, K]`
per-chain statistics of two half-windows; `combine` turns those few numbers into the diagnostics on the host.  The same
pair serves stored parameter chains, the log-posterior trace (K = 1) and predictions of thinned draws (function-space
diagnostics: weight-space R-hat of a neural network is pessimistic, hidden units can be permuted).

Definitions: classic split-R-hat (Gelman et al., Bayesian Data Analysis, 3rd ed., section 11.4) over the m = 2C half
chains, and the batch-means estimate of the effective sample size (Flegal & Jones, Ann. Statist. 38, 2010) with batches
of floor(sqrt(n)) draws.  Both need one pass and neither a sort nor an FFT.  Rank-normalised / folded R-hat (Vehtari et
al. 2021) and autocorrelation-based ESS are in `rankdiag.py` (`qn_rank_diag`, csrc/qn_rank.hip), which sorts the pooled
draws of every entry.  The reference runs one chain and has no counterpart.
"""
import math

import numpy as np
import torch

from .. import _lib

# host chains are uploaded in pieces of whole chains of at most this many bytes (one chain if a single one is larger)
DEFAULT_UPLOAD_BYTES = 1 << 30


def batch_plan(T, nburn=0):
    """`(t0, nbatch, blen)` of a chain of T rows after `nburn` burn-in rows: the two halves have
    `half = (T - nburn) // 2` rows at most, batches of `blen = floor(sqrt(half))` rows, `nbatch = half // blen` batches
    per half, and the LAST `2 * nbatch * blen` rows are used (`t0 = T - 2 * nbatch * blen >= nburn`).
    ValueError if `nburn` is outside [0, T) or fewer than 8 rows remain (two halves of two batches of two rows is the
    least that is accepted; it implies nbatch >= 2)."""
    T, nburn = int(T), int(nburn)
    if not 0 <= nburn < T:
        raise ValueError(f"nburn = {nburn} outside [0, T = {T})")
    half = (T - nburn) // 2
    blen = math.isqrt(half)
    nbatch = half // blen if blen else 0
    if T - nburn < 8 or nbatch < 2:
        raise ValueError(f"{T - nburn} rows after burn-in: diagnostics need at least 8 (two halves of two batches of two)")
    return T - 2 * nbatch * blen, nbatch, blen


def _device_stats(t, t0, nbatch, blen):
    C, T, K = t.shape
    L = _lib.lib()
    need = L.qn_chain_stats_workspace_bytes(C, T, K, nbatch, blen)
    if need == 0:
        raise ValueError(L.qn_last_error().decode())
    stats = torch.empty(C, 6, K, dtype=torch.float64, device=t.device)
    ws = torch.empty(need // 8, dtype=torch.float64, device=t.device)
    qdt = _lib.QN_F32 if t.dtype == torch.float32 else _lib.QN_F64
    with torch.cuda.device(t.device):
        st = _lib.stream(t.device)
        _lib.check(L.qn_chain_stats(t.data_ptr(), qdt, C, T, K, t0, nbatch, blen, stats.data_ptr(), ws.data_ptr(), need, st),
                   "qn_chain_stats")
    return stats


def chain_stats(chain, nburn=0, device=None, max_upload_bytes=DEFAULT_UPLOAD_BYTES):
    """Device tensor `[C, 6, K]` float64 of `qn_chain_stats` (include/quinn_amd.h) for the window `batch_plan(T, nburn)`.

    chain `[C, T, K]` (or `[T, K]`: one chain), float64 or float32:
      a device tensor -- read where it is (it must be contiguous; nothing is copied);
      a numpy array / host tensor -- uploaded to `device` (default: the current one) in pieces of whole chains of at
        most `max_upload_bytes`, window rows only; the statistics of a chain do not depend on the other chains, so the
        pieces concatenate exactly and a host array larger than device memory never needs a device copy of itself.
    """
    if isinstance(chain, torch.Tensor) and chain.is_cuda:
        t = chain if chain.dim() == 3 else chain.unsqueeze(0)
        if t.dim() != 3 or t.dtype not in (torch.float64, torch.float32) or not t.is_contiguous():
            raise ValueError("chain: a contiguous [C, T, K] float64 / float32 tensor is needed")
        t0, nbatch, blen = batch_plan(t.shape[1], nburn)
        if t.shape[0] == 0:
            return torch.empty(0, 6, t.shape[2], dtype=torch.float64, device=t.device)
        return _device_stats(t, t0, nbatch, blen)
    a = chain.numpy() if isinstance(chain, torch.Tensor) else np.asarray(chain)
    if a.dtype not in (np.float64, np.float32):
        a = a.astype(np.float64)
    if a.ndim == 2:
        a = a[None]
    if a.ndim != 3:
        raise ValueError("chain: [C, T, K] (or [T, K]) is needed")
    C, T, K = a.shape
    t0, nbatch, blen = batch_plan(T, nburn)
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    if C == 0:
        return torch.empty(0, 6, K, dtype=torch.float64, device=dev)
    per = max(1, int(max_upload_bytes) // max(1, (T - t0) * K * a.itemsize))
    out = []
    for lo in range(0, C, per):
        piece = torch.as_tensor(np.ascontiguousarray(a[lo:lo + per, t0:])).to(dev)
        out.append(_device_stats(piece, 0, nbatch, blen))
    return out[0] if len(out) == 1 else torch.cat(out)


def combine(stats, nbatch, blen, t0=None):
    """Split-R-hat, ESS and pooled moments from `[C, 6, K]` chain statistics (device tensor or array), numpy float64.

    With m = 2C sequences (the halves) of n = nbatch * blen draws and s2_j = M2_j / (n - 1):
      W = mean_j s2_j,  B = n var_j(mean_j, ddof=1),  var = (n - 1) / n W + B / n,  rhat = sqrt(var / W),
      sigma2 = mean_j [ blen Sb_j / (nbatch - 1) ]  (batch-means estimate of the asymptotic variance),
      ess = m n var / sigma2.
    Keys: rhat, ess, mean (of the m means), var `[K]`; chain_mean, chain_var (ddof=1, the two halves merged exactly)
    `[C, K]`; n_draws (= m n), nbatch, blen, t0.  An entry no chain ever moved (W = 0) gives NaN, silently."""
    s = stats.detach().cpu().numpy() if isinstance(stats, torch.Tensor) else np.asarray(stats)
    s = np.asarray(s, dtype=np.float64)
    if s.ndim != 3 or s.shape[1] != 6 or s.shape[0] < 1:
        raise ValueError("stats: [C, 6, K] with C >= 1 is needed")
    C, _, K = s.shape
    nbatch, blen = int(nbatch), int(blen)
    n, m = nbatch * blen, 2 * C
    means = s[:, 0:2].reshape(m, K)
    M2 = s[:, 2:4].reshape(m, K)
    Sb = s[:, 4:6].reshape(m, K)
    with np.errstate(divide="ignore", invalid="ignore"):
        W = (M2 / (n - 1)).mean(axis=0)
        B = n * means.var(axis=0, ddof=1)
        var = (n - 1) / n * W + B / n
        rhat = np.sqrt(var / W)
        sigma2 = (blen * Sb / (nbatch - 1)).mean(axis=0)
        ess = m * n * var / sigma2
        cmean = 0.5 * (s[:, 0] + s[:, 1])
        cvar = (s[:, 2] + s[:, 3] + 0.5 * n * (s[:, 0] - s[:, 1]) ** 2) / (2 * n - 1)
    return {"rhat": rhat, "ess": ess, "mean": means.mean(axis=0), "var": var, "chain_mean": cmean, "chain_var": cvar,
            "n_draws": m * n, "nbatch": nbatch, "blen": blen, "t0": None if t0 is None else int(t0)}


def diagnose_chains(chain, nburn=0, n_total=None, gather="all", device=None):
    """`combine(chain_stats(chain, nburn))`.  Multi-rank runs pass this rank's shard of the chains and `n_total`: the small
    `[C_local, 6, K]` statistics are gathered with `parallel.gather_rows(..., dst=gather)` and combined (on the ranks
    that receive them; the others combine their own shard; a rank left without any chain gets None)."""
    from ..parallel import dist_info, gather_rows
    T = chain.shape[-2]
    t0, nbatch, blen = batch_plan(T, nburn)
    stats = chain_stats(chain, nburn, device=device)
    if n_total is not None and dist_info()[1] > 1:
        stats = gather_rows(stats, n_total, dst=gather)
    if stats.shape[0] == 0:
        return None
    return combine(stats, nbatch, blen, t0)


# ---- row selection of predictive ensembles (pure index logic) ---------------------------------------------------------------
def thinned_rows(T, nens, nburn):
    """The reference's thinning rule (nn_mcmc.py:194-199): rows nburn + j * int((T - nburn) / nens), j < nens."""
    nevery = int((T - nburn) / nens)
    return [nburn + j * nevery for j in range(nens)]


def pooled_rows(C, T, nens, nburn):
    """`[(chain, rows)]` of an `nens`-member ensemble pooled over C chains: chain c contributes
    `nens // C + (c < nens % C)` draws, thinned by the reference's rule with that per-chain count; chain-major order.
    Chains whose share is zero (nens < C) are left out."""
    out = []
    for c in range(C):
        cnt = nens // C + (1 if c < nens % C else 0)
        if cnt > 0:
            out.append((c, thinned_rows(T, cnt, nburn)))
    return out
