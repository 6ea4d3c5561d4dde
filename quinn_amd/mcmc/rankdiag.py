"""Rank-normalised split-R-hat, folded R-hat, bulk- and tail-ESS and the MCSE of the mean (Vehtari, Gelman, Simpson, Carpenter
& Buerkner, Bayesian Analysis 16, 2021) of many chains.

`rank_rows` is the contract in numpy float64 and the authority of the device pass `qn_rank_diag` (csrc/qn_rank.hip,
include/quinn_amd_rank.h); `rank_stats` runs the device pass.  They complement `diagnostics.py` (classic split-R-hat, batch-means
ESS), which does not see chains that agree in mean and differ in scale and means nothing for heavy tails.

The window.  `chain [C, T, K]`; a plan `(t0, nh, stride)` uses rows `t0 + j * stride`, `j < 2 nh`, of every chain; `j // nh` is
the half, so there are `m = 2 C` split sequences of `nh` draws (sequence `2 c + h`) and `S = 2 C nh` pooled draws, at most
QN_RANK_MAX_S: a longer chain is THINNED by `stride`, and every ESS below is that of the thinned draws (`n_draws = S` and
`stride` are returned with them).

Per entry, with x the S window values and s the same sorted:
  ranks     r_i = (#{x_j < x_i} + #{x_j <= x_i} + 1) / 2 (average ranks, ties exact), z_i = Phi^-1((r_i - 3/8) / (S + 1/4)), Phi^-1
            being `statistics.NormalDist().inv_cdf`.
  R-hat     of a series v over the m sequences, as `diagnostics.combine`: with d = v - v_0 (a common shift, exact in real
            arithmetic, that keeps a large offset out of the sums), mean_j and the centred c_ji = d_ji - mean_j,
            W = mean_j sum_i c_ji^2 / (nh - 1),  B = nh var_j(mean_j, ddof=1),  var+ = (nh - 1) / nh W + B / nh,  sqrt(var+ / W).
            rhat_bulk is that of z; rhat_tail that of the rank-normalised |x - med|, med = (s[(S-1)//2] + s[S//2]) / 2.
  ESS       of a series v (section 3.2 of the paper, as in Stan >= 2.21 and ArviZ):
            A_t = mean_j (1 / nh) sum_{i < nh - t} c_ji c_j,i+t  (biased autocovariance by the direct sum; W = A_0 nh / (nh - 1)),
            rho_0 = 1, rho_t = 1 - (W - A_t) / var+,  pair sums P_k = rho_2k + rho_2k+1 for k < nh // 2;
            k* = the first k >= 1 with P_k <= 0 (Geyer's initial positive sequence), nh // 2 if there is none;
            P'_0 = P_0, P'_k = min(P'_k-1, P_k) (the monotone correction);
            tau = -1 + 2 sum_{k < k*} P'_k + max(rho_2k*, 0) (the last term only if the sequence stopped),
            tau = max(tau, 1 / log10(S)),  ess = S / tau.
            Every decision is taken at 0 on the quantity it admits: a pair enters when its sum is positive, and at 0 it -- and
            after the monotone correction every later pair, each at most the one before -- adds nothing; the trailing
            even-lag term enters when it is positive.  A rounding error therefore moves tau by its own size, not by a jump,
            except that the trailing term is read at the pair that stopped: two evaluations that stop at different pairs
            (a pair sum within rounding of 0) can differ by that term.
            ess_bulk = ess(z),  ess_tail = min(ess(1[x <= q05]), ess(1[x <= q95])) with q the pooled quantile at position
            q (S - 1) of s, linearly interpolated,  ess_mean = ess(x),  mcse_mean = sqrt(var(x, ddof=1) / ess_mean).
  NaN       an entry with a non-finite value anywhere in its window: all six figures; a series without within-sequence
            variance (W = 0): the figures built on it (as `combine`).  No other entry is touched.
"""
import statistics

import numpy as np
import torch

from .. import _lib

QN_RANK_MAX_S = _lib.RANK_MAX_S
KEYS = ("rhat_bulk", "rhat_tail", "ess_bulk", "ess_tail", "ess_mean", "mcse_mean")      # the rows of qn_rank_diag, in order
_LAG_BLOCK = 32          # lags the contract forms at a time (the figures do not depend on it)


def rank_plan(C, T, nburn=0, max_draws=None):
    """`(t0, nh, stride)`: nh = min((T - nburn) // 2, max_draws // (2 C)) draws per half, stride = (T - nburn) // (2 nh), and
    the window ends on the last row, t0 = T - 1 - (2 nh - 1) stride (>= nburn by construction).  max_draws defaults to
    QN_RANK_MAX_S.  ValueError if nburn is outside [0, T) or nh < 4."""
    C, T, nburn = int(C), int(T), int(nburn)
    max_draws = QN_RANK_MAX_S if max_draws is None else int(max_draws)
    if C < 1 or not 0 <= nburn < T:
        raise ValueError(f"C = {C} chains, nburn = {nburn} outside [0, T = {T})")
    nh = min((T - nburn) // 2, max_draws // (2 * C))
    if nh < 4:
        raise ValueError(f"{T - nburn} rows after burn-in and at most {max_draws} pooled draws of {C} chains: rank diagnostics need "
                         "nh >= 4 draws per half")
    stride = (T - nburn) // (2 * nh)
    return T - 1 - (2 * nh - 1) * stride, nh, stride


def window(chain, t0, nh, stride):
    """`[m, nh, K]` float64: the split sequences of the plan, sequence 2 c + h."""
    a = np.asarray(chain)
    C, T, K = a.shape
    w = a[:, t0:t0 + (2 * nh - 1) * stride + 1:stride, :]
    return np.ascontiguousarray(w, dtype=np.float64).reshape(2 * C, nh, K)


def twice_ranks(x):
    """`#{x_j < x_i} + #{x_j <= x_i} + 1` (twice the average rank, an integer) along axis 0 of `[S, K]`, and the sorted
    columns."""
    s = np.sort(x, axis=0)
    r2 = np.empty(x.shape, dtype=np.int64)
    for k in range(x.shape[1]):
        r2[:, k] = np.searchsorted(s[:, k], x[:, k], "left") + np.searchsorted(s[:, k], x[:, k], "right") + 1
    return r2, s


def rank_normalise(x):
    """`(z, sorted x)` of `[S, K]`: z = Phi^-1((r - 3/8) / (S + 1/4)) of the average ranks r."""
    S = x.shape[0]
    r2, s = twice_ranks(x)
    u, inv = np.unique(r2, return_inverse=True)
    inv_cdf = statistics.NormalDist().inv_cdf
    zu = np.array([inv_cdf(float((0.5 * v - 0.375) / (S + 0.25))) for v in u])
    return zu[inv].reshape(x.shape), s


def sorted_quantile(s, q):
    """The quantile at position q (S - 1) of the sorted columns `s [S, K]`, linearly interpolated."""
    S = s.shape[0]
    pos = q * float(S - 1)
    i0 = int(pos)
    i1 = min(i0 + 1, S - 1)
    return s[i0] + (pos - float(i0)) * (s[i1] - s[i0])


def _centred(v):
    """(c [m, nh, K], mean_j [m, K]) of d = v - v[0, 0]."""
    d = v - v[0, 0]
    mean = d.sum(axis=1) / v.shape[1]
    return d - mean[:, None, :], mean


def _w_b(c, mean):
    m, nh, _ = c.shape
    with np.errstate(invalid="ignore"):
        A0 = (c * c).sum(axis=1).sum(axis=0) / nh / m
        W = A0 * nh / (nh - 1.0)
        B = nh * ((mean - mean.sum(axis=0) / m) ** 2).sum(axis=0) / (m - 1.0)
        ok = W > 0
    return np.where(ok, W, np.nan), np.where(ok, B, np.nan)


def split_rhat(v):
    """Split-R-hat `[K]` of the series `v [m, nh, K]` (the module docstring has the formulas); NaN where W = 0."""
    nh = v.shape[1]
    W, B = _w_b(*_centred(v))
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.sqrt(((nh - 1.0) / nh * W + B / nh) / W)


def ess(v):
    """The autocorrelation ESS `[K]` of the series `v [m, nh, K]` (the module docstring has the steps); NaN where W = 0."""
    m, nh, K = v.shape
    S = m * nh
    c, mean = _centred(v)
    W, B = _w_b(c, mean)
    varp = (nh - 1.0) / nh * W + B / nh
    npair = nh // 2
    active = np.isfinite(W)                 # entries whose sequence has not stopped
    sumP, prev, trail = np.zeros(K), np.zeros(K), np.zeros(K)
    for l0 in range(0, 2 * npair, _LAG_BLOCK):
        if not active.any():
            break
        ca = c[:, :, active]
        A = np.stack([(ca[:, :nh - t] * ca[:, t:]).sum(axis=1).sum(axis=0) / nh / m if t < nh else np.zeros(ca.shape[2])
                      for t in range(l0, l0 + _LAG_BLOCK)])
        idx = np.flatnonzero(active)
        rho = 1.0 - (W[idx] - A) / varp[idx]
        live = np.ones(len(idx), dtype=bool)
        for i in range(0, _LAG_BLOCK, 2):
            k = (l0 + i) // 2
            if k >= npair:
                break
            re = np.ones(len(idx)) if k == 0 else rho[i]
            P = re + rho[i + 1]
            if k == 0:
                sumP[idx], prev[idx] = P, P
                continue
            go = live & (P > 0)
            stop = live & ~go
            pk = np.minimum(prev[idx], P)
            prev[idx[go]] = pk[go]
            sumP[idx[go]] += pk[go]
            trail[idx[stop]] = np.maximum(re[stop], 0.0)
            live &= go
        active[idx[~live]] = False
    tau = np.maximum(-1.0 + 2.0 * sumP + trail, 1.0 / np.log10(S))
    return np.where(np.isfinite(W), S / tau, np.nan)


def rank_rows(chain, t0, nh, stride):
    """`[6, K]` float64, the rows of `qn_rank_diag` in the order of KEYS, of `chain [C, T, K]` and the plan: the contract."""
    xw = window(chain, t0, nh, stride)
    m, _, K = xw.shape
    S = m * nh
    out = np.full((6, K), np.nan)
    good = np.isfinite(xw).all(axis=(0, 1))
    if not good.any():
        return out
    xw = xw[:, :, good]
    x = xw.reshape(S, -1)
    z, s = rank_normalise(x)
    med = 0.5 * (s[(S - 1) // 2] + s[S // 2])
    zf, _ = rank_normalise(np.abs(x - med))
    shape = xw.shape
    ind = [(x <= sorted_quantile(s, q)).astype(np.float64).reshape(shape) for q in (0.05, 0.95)]
    ess_mean = ess(xw)
    with np.errstate(invalid="ignore"):
        rows = [split_rhat(z.reshape(shape)), split_rhat(zf.reshape(shape)), ess(z.reshape(shape)),
                np.minimum(ess(ind[0]), ess(ind[1])), ess_mean, np.sqrt(x.var(axis=0, ddof=1) / ess_mean)]
    out[:, good] = np.stack(rows)
    return out


def _as_dict(rows, C, t0, nh, stride):
    d = {k: rows[i] for i, k in enumerate(KEYS)}
    d["rhat_rank"] = np.maximum(d["rhat_bulk"], d["rhat_tail"])
    d.update(n_draws=2 * C * nh, nh=nh, stride=stride, t0=t0)
    return d


def rank_stats_host(chain, nburn=0, max_draws=None):
    """`rank_stats` by the numpy contract (no device)."""
    a = np.asarray(chain)
    a = a[None] if a.ndim == 2 else a
    t0, nh, stride = rank_plan(a.shape[0], a.shape[1], nburn, max_draws)
    return _as_dict(rank_rows(a, t0, nh, stride), a.shape[0], t0, nh, stride)


def _device_rows(t, t0, nh, stride):
    """`[6, K]` device tensor of qn_rank_diag on the contiguous device tensor `t [C, T, K]`."""
    C, T, K = t.shape
    L = _lib.lib()
    need = L.qn_rank_diag_workspace_bytes(C, T, K, nh, stride)
    if need == 0:
        raise ValueError(L.qn_last_error().decode())
    out = torch.empty(_lib.RANK_NOUT, K, dtype=torch.float64, device=t.device)
    ws = torch.empty(need // 8, dtype=torch.float64, device=t.device)
    qdt = _lib.QN_F32 if t.dtype == torch.float32 else _lib.QN_F64
    with torch.cuda.device(t.device):
        st = _lib.stream(t.device)
        _lib.check(L.qn_rank_diag(t.data_ptr(), qdt, C, T, K, t0, nh, stride, out.data_ptr(), ws.data_ptr(), need, st), "qn_rank_diag")
    return out


def rank_stats(chain, nburn=0, max_draws=None, device=None, max_bytes=256 << 20):
    """The rank diagnostics of `chain [C, T, K]` (or `[T, K]`: one chain), float64 or float32, after `nburn` rows, by the device
    pass: a dict of numpy arrays `[K]` rhat_bulk, rhat_tail, rhat_rank (the larger of the two), ess_bulk, ess_tail, ess_mean,
    mcse_mean, and the plan n_draws (= S), nh, stride, t0 of `rank_plan(C, T, nburn, max_draws)`.  With stride > 1 the ESS
    values are those of the thinned draws.
      a device tensor -- read where it is (contiguous; nothing is copied) when the call's workspace fits `max_bytes`, else
        the window rows of column chunks are copied and passed one after the other;
      a numpy array / host tensor -- window rows only are uploaded to `device` (default: the current one), in chunks of K
        such that a chunk and its workspace stay within `max_bytes`.
    An entry's figures do not depend on the other entries, so the chunks concatenate exactly."""
    on_dev = isinstance(chain, torch.Tensor) and chain.is_cuda
    a = chain if on_dev else (chain.numpy() if isinstance(chain, torch.Tensor) else np.asarray(chain))
    if not on_dev and a.dtype not in (np.float64, np.float32):
        a = a.astype(np.float64)
    if on_dev and a.dtype not in (torch.float64, torch.float32):
        raise ValueError("chain: float64 or float32 is needed")
    if a.ndim == 2:
        a = a[None]
    if a.ndim != 3 or a.shape[2] < 1:
        raise ValueError("chain: [C, T, K] (or [T, K]) with K >= 1 is needed")
    C, T, K = a.shape
    t0, nh, stride = rank_plan(C, T, nburn, max_draws)
    S = 2 * C * nh
    L = _lib.lib()
    if on_dev and a.is_contiguous() and 0 < L.qn_rank_diag_workspace_bytes(C, T, K, nh, stride) <= max_bytes:
        rows = _device_rows(a, t0, nh, stride).cpu().numpy()
        return _as_dict(rows, C, t0, nh, stride)
    dev = a.device if on_dev else (torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device()))
    kc = max(1, int(max_bytes) // (S * 8 * 3))          # the chunk's window and the two workspace rows of an entry
    win = slice(t0, t0 + (2 * nh - 1) * stride + 1, stride)
    pieces = []
    for k0 in range(0, K, kc):
        if on_dev:
            piece = a[:, win, k0:k0 + kc].contiguous()
        else:
            piece = torch.as_tensor(np.ascontiguousarray(a[:, win, k0:k0 + kc])).to(dev)
        pieces.append(_device_rows(piece, 0, nh, 1).cpu().numpy())
    return _as_dict(np.concatenate(pieces, axis=1), C, t0, nh, stride)
