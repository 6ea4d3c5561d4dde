"""Laplace evidence in numpy: the contract of `qn_la_evidence` and `qn_la_tune` (csrc/qn_evidence.hip,
include/quinn_amd_evidence.h), and their wrappers on torch tensors.

Float64 numpy and the authority for the device kernels, as stacking.py is for `qn_stack_weights`; `log_evidence` and `tune` take
`dtype=` and run in np.longdouble too.  MacKay (Neural Comput. 4, 1992), Immer et al. (ICML 2021).  The reference has no
counterpart.

Per member, at its MAP weights w [p]: c [p] >= 0 is the spectrum of the curvature in units of G (H = G / s2 + diag(tau)),
sse the sum of squared errors over the n entries of y on its rows, and the groups g = 0 .. G - 1 are the contiguous segments
bounds[g] .. bounds[g + 1] - 1 (n_g elements).  With the noise variance s2 and the precisions tau_g:

    lambda_j = c_j / s2 + tau_g(j)        logdet = sum_j log lambda_j
    gamma_g  = sum_{j in g} (c_j / s2) / lambda_j       gamma = sum_g gamma_g         (the effective number of parameters)
    S_g      = sum_{j in g} w_j^2
    loglik   = -n/2 log(2 pi s2) - sse / (2 s2)
    logZ     = loglik + sum_g (n_g/2 log tau_g - tau_g S_g / 2) - logdet / 2

(the (2 pi)^(p/2) of the Gaussian integral cancels the prior's normaliser; `cov_scale` plays no part).  The rows of a result are
`ROWS`, then gamma_g [G], then S_g [G].  An s2 or tau_g that is not finite and > 0, a c_j that is negative or not finite, a w_j
or sse that is not finite makes every row NaN.

d logZ / d log tau_g = (gamma_g - tau_g S_g) / 2 and d logZ / d log s2 = (sse / s2 - (n - gamma)) / 2, so the stationary points
are MacKay's fixed point tau_g S_g = gamma_g, s2 (n - gamma) = sse; `tune` iterates it, see there.
"""
import numpy as np

from .mcmc.hyper import check_segments, group_segments

ROWS = ("logZ", "loglik", "logdet", "gamma")
STATUS = ("iters", "returned", "converged", "resid", "logZ_start", "clamped")       # qn_la_tune's status block
CLAMP_S2_MIN, CLAMP_S2_MAX, CLAMP_TAU_MIN, CLAMP_TAU_MAX = 1, 2, 4, 8               # the bits of `clamped`
DEFAULT_TOL = 1e-8
DEFAULT_MAX_ITER = 1000
MAX_ITER = 100000
DEFAULT_CLAMPS = dict(s2_min=1e-12, s2_max=1e12, tau_min=1e-12, tau_max=1e12)
EVIDENCE_TYPES = ('ggn', 'ggn_diag', 'kron')


def kron_spectrum(lamS, lamA, nb):
    """c `[..., p]` of a Kronecker-factored curvature: for the layers i in order, lamS[i] `[..., h_{i+1}]` and lamA[i]
    `[..., e_i]` (the factors' eigenvalues, clamped at 0) give c[(i, a, b)] = lamS_i[a] lamA_i[b] / nb in the `[h_{i+1}, e_i]`
    order at the offsets `KronLayout.offK` -- the order of `Dinv`.  numpy arrays or torch tensors."""
    blocks = [(s[..., :, None] * a[..., None, :] / nb).reshape(*s.shape[:-1], -1) for s, a in zip(lamS, lamA)]
    if isinstance(blocks[0], np.ndarray):
        return np.concatenate(blocks, axis=-1)
    import torch
    return torch.cat(blocks, dim=-1)


def check_groups(la_type, groups):
    """ValueError unless the Laplace type has a spectrum that the precisions of `groups` commute with."""
    if la_type not in EVIDENCE_TYPES:
        raise ValueError(f"the evidence is defined for la_type 'ggn', 'ggn_diag' and 'kron', not for {la_type!r} "
                         "(the reference's types have a hard-wired noise and no prior)")
    if groups not in ('layer', 'tensor', 'all'):
        raise ValueError(f"groups = {groups!r} is 'layer', 'tensor' or 'all'")
    if la_type == 'kron' and groups == 'tensor':
        raise ValueError("la_type 'kron' takes groups 'layer' or 'all': a weight and its bias share A_i's eigenbasis")
    if la_type == 'ggn' and groups != 'all':
        raise ValueError("la_type 'ggn' takes groups 'all' only: a per-layer precision does not commute with a dense G")


def group_bounds(arch, groups):
    """(bounds int64 `[G + 1]`, names) of the groups 'layer' | 'tensor' | 'all' of an `MLPArch` in its flat weight order: those
    of `hyperprior` (`mcmc.hyper.group_segments`).  A layer's block has the same bounds in kron order."""
    return group_segments(arch, groups)


def _prep(c, bounds, W, sse, s2, tau, dtype):
    c = np.asarray(c).astype(dtype)
    bounds = check_segments(bounds, c.shape[-1])
    G = len(bounds) - 1
    W = np.asarray(W).astype(dtype)
    sse, s2 = np.asarray(sse).astype(dtype), np.asarray(s2).astype(dtype)
    tau = np.asarray(tau).astype(dtype)
    if tau.shape[-1:] != (G,):
        raise ValueError(f"tau of shape {tau.shape}: {G} precisions in the last axis are needed")
    return c, bounds, G, W, sse, s2, tau


def log_evidence(c, bounds, W, sse, n, s2, tau, dtype=np.float64):
    """`[..., 4 + 2 G]` in `dtype`: logZ, loglik, logdet, gamma, gamma_g [G], S_g [G] (the module docstring) for c, W `[..., p]`,
    sse, s2 `[...]` and tau `[..., G]`, broadcast against each other in the leading axes."""
    c, bounds, G, W, sse, s2, tau = _prep(c, bounds, W, sse, s2, tau, dtype)
    lead = np.broadcast_shapes(c.shape[:-1], W.shape[:-1], sse.shape, s2.shape, tau.shape[:-1])
    out = np.empty(lead + (len(ROWS) + 2 * G,), dtype=dtype)
    ng = np.diff(bounds).astype(dtype)
    two_pi = dtype(8) * np.arctan(dtype(1))
    with np.errstate(all="ignore"):
        bad = ~(np.isfinite(s2) & (s2 > 0)) | ~np.isfinite(sse) | np.any(~(np.isfinite(tau) & (tau > 0)), axis=-1) | \
            np.any(~(np.isfinite(c) & (c >= 0)), axis=-1) | np.any(~np.isfinite(W), axis=-1)
        a = c / s2[..., None]
        lam = a + np.repeat(tau, np.diff(bounds), axis=-1)
        loglam, ratio, w2 = np.log(lam), a / lam, W * W
        logdet = np.zeros(lead, dtype=dtype)
        for g, (lo, hi) in enumerate(zip(bounds[:-1], bounds[1:])):
            logdet = logdet + loglam[..., lo:hi].sum(axis=-1)
            out[..., len(ROWS) + g] = ratio[..., lo:hi].sum(axis=-1)
            out[..., len(ROWS) + G + g] = w2[..., lo:hi].sum(axis=-1)
        gam_g, S_g = out[..., len(ROWS):len(ROWS) + G], out[..., len(ROWS) + G:]
        loglik = -dtype(0.5) * dtype(n) * np.log(two_pi * s2) - dtype(0.5) * sse / s2
        out[..., 0] = loglik + (dtype(0.5) * ng * np.log(tau) - dtype(0.5) * tau * S_g).sum(axis=-1) - dtype(0.5) * logdet
        out[..., 1] = loglik
        out[..., 2] = logdet
        out[..., 3] = gam_g.sum(axis=-1)
    out[np.broadcast_to(bad, lead)] = np.nan
    return out


def residual(rows, G, sse, n, s2, tau, tune_noise=True, tune_prior=True):
    """The stopping rule's resid of ONE member from its rows at (s2, tau `[G]`):
    max(max_g |log(gamma_g / (tau_g S_g))| (tune_prior), |log(sse / ((n - gamma) s2))| (tune_noise)), 0 if nothing is tuned; an
    argument of a log that is not finite and > 0 makes it +Inf."""
    dtype = rows.dtype.type
    args = []
    with np.errstate(all="ignore"):
        if tune_prior:
            args += list(rows[len(ROWS):len(ROWS) + G] / (tau * rows[len(ROWS) + G:]))
        if tune_noise:
            args.append(sse / ((dtype(n) - rows[3]) * s2))
        if not args:
            return dtype(0)
        args = np.asarray(args, dtype=rows.dtype)
        if not np.all(np.isfinite(args) & (args > 0)):
            return dtype(np.inf)
        return np.max(np.abs(np.log(args)))


def tune(c, bounds, W, sse, n, s2_0, tau_0, tol=DEFAULT_TOL, max_iter=DEFAULT_MAX_ITER, tune_noise=True, tune_prior=True,
         s2_min=DEFAULT_CLAMPS['s2_min'], s2_max=DEFAULT_CLAMPS['s2_max'], tau_min=DEFAULT_CLAMPS['tau_min'],
         tau_max=DEFAULT_CLAMPS['tau_max'], dtype=np.float64, trace=False):
    """MacKay's fixed point for ONE member (c, W `[p]`, tau_0 `[G]`), step by step as `qn_la_tune` runs it.  A dict with `s2`,
    `tau` `[G]`, `rows` (of the returned iterate), the `STATUS` entries and, with trace=True, `logZs` and `resids` of every
    iterate evaluated.

    Iterate t = 0, 1, ... evaluates the rows and `residual` at theta_t = (s2, tau).
      resid <= tol:   stop, converged = 1, theta_t is the answer.
      t == max_iter:  stop, converged = 0, the answer is the evaluated iterate with the largest finite logZ (the first on a tie;
                      iterate 0 if none was finite), so logZ >= logZ_start.
      otherwise       s2   <- sse / (n - gamma) clamped to [s2_min, s2_max]; s2_max if n - gamma <= 0            (tune_noise)
                      tau_g <- gamma_g / S_g clamped to [tau_min, tau_max]; tau_min if gamma_g <= 0, else tau_max if S_g == 0
                                                                                                                  (tune_prior)
                      and a clamp that acts sets its bit in `clamped`.
    A member whose inputs are bad (`log_evidence`'s rules) gets NaN rows, its start back, iters = converged = 0, resid = +Inf."""
    if not (tol >= 0 and np.isfinite(tol)) or not 0 <= int(max_iter) <= MAX_ITER:
        raise ValueError(f"tune: tol = {tol!r} is finite and >= 0, max_iter = {max_iter!r} is in 0 .. {MAX_ITER}")
    if not (0 < s2_min <= s2_max < np.inf and 0 < tau_min <= tau_max < np.inf):
        raise ValueError("tune: the clamps are finite with 0 < min <= max")
    c, bounds, G, W, sse, s2, tau = _prep(c, bounds, W, sse, s2_0, tau_0, dtype)
    if c.ndim != 1 or W.shape != c.shape or tau.shape != (G,) or sse.ndim or s2.ndim:
        raise ValueError("tune takes one member: c, W [p], tau_0 [G], scalar sse and s2_0")
    tau = tau.copy()
    nn = dtype(n)
    res = {}
    rows = log_evidence(c, bounds, W, sse, n, s2, tau, dtype)
    if np.isnan(rows[0]) and np.all(np.isnan(rows)):
        res.update(s2=s2, tau=tau, rows=rows, iters=0, returned=0, converged=0, resid=dtype(np.inf), logZ_start=dtype(np.nan),
                   clamped=0)
        if trace:
            res.update(logZs=np.array([np.nan]), resids=np.array([np.inf]))
        return res
    flags, best, logZs, resids = 0, None, [], []
    t = 0
    with np.errstate(all="ignore"):
        while True:
            if t > 0:
                rows = log_evidence(c, bounds, W, sse, n, s2, tau, dtype)
            resid = residual(rows, G, sse, n, s2, tau, tune_noise, tune_prior)
            logZs.append(rows[0])
            resids.append(resid)
            if t == 0 or (np.isfinite(rows[0]) and not best[0][0] >= rows[0]):
                best = (rows, resid, s2, tau.copy(), t)
            conv = bool(resid <= tol)
            if conv or t >= max_iter:
                break
            gam_g, S_g = rows[len(ROWS):len(ROWS) + G], rows[len(ROWS) + G:]
            if tune_noise:
                den = nn - rows[3]
                v = sse / den if den > 0 else dtype(s2_max)
                if not den > 0 or v > s2_max:
                    v, flags = dtype(s2_max), flags | CLAMP_S2_MAX
                elif v < s2_min:
                    v, flags = dtype(s2_min), flags | CLAMP_S2_MIN
                s2 = v
            if tune_prior:
                new = tau.copy()
                for g in range(G):
                    if not gam_g[g] > 0:
                        new[g], flags = tau_min, flags | CLAMP_TAU_MIN
                    elif S_g[g] == 0 or gam_g[g] / S_g[g] > tau_max:
                        new[g], flags = tau_max, flags | CLAMP_TAU_MAX
                    elif gam_g[g] / S_g[g] < tau_min:
                        new[g], flags = tau_min, flags | CLAMP_TAU_MIN
                    else:
                        new[g] = gam_g[g] / S_g[g]
                tau = new
            t += 1
    returned = t
    if not conv:
        rows, resid, s2, tau, returned = best
    res.update(s2=s2, tau=tau, rows=rows, iters=t, returned=returned, converged=int(conv), resid=resid, logZ_start=logZs[0],
               clamped=flags)
    if trace:
        res.update(logZs=np.array(logZs, dtype=dtype), resids=np.array(resids, dtype=dtype))
    return res


def synthetic_member(p, G, n, nonzero=None, seed=0, log_mean=1.0, log_sd=2.0):
    """(c [p], bounds [G + 1], W [p], sse) of a made-up member for tests and benchmarks: `nonzero` (default p) log-normal
    c_j = exp(log_mean + log_sd z) at random places, the others 0, W ~ 0.5 N(0, 1), sse ~ 0.01 chi^2_n, G groups with random
    interior bounds.  Seeded; nothing else is random."""
    rs = np.random.RandomState(seed)
    nz = p if nonzero is None else int(nonzero)
    c = np.zeros(p)
    c[rs.permutation(p)[:nz]] = np.exp(rs.randn(nz) * log_sd + log_mean)
    W = 0.5 * rs.randn(p)
    sse = 0.01 * rs.chisquare(n)
    bounds = np.r_[0, np.sort(rs.permutation(np.arange(1, p))[:G - 1]), p] if G > 1 else np.array([0, p])
    return c, bounds.astype(np.int64), W, float(sse)


def softmax_weights(logZ):
    """The members' evidence weights: softmax of logZ `[M]` (numpy float64).  A member whose logZ is NaN or -Inf gets weight 0;
    ValueError if no member has a finite logZ."""
    z = np.asarray(logZ, dtype=np.float64).reshape(-1)
    ok = np.isfinite(z)
    if not ok.any():
        raise ValueError("evidence weights need at least one member with a finite log evidence")
    w = np.zeros_like(z)
    w[ok] = np.exp(z[ok] - z[ok].max())
    return w / w.sum()


# ---------------------------------------------------------------------------------------------------- the device calls
def _dev_args(what, c, W, sse, bounds):
    import torch
    if not isinstance(c, torch.Tensor) or c.dtype != torch.float64 or c.dim() != 2 or not c.is_contiguous() or not c.is_cuda:
        raise ValueError(f"{what}: c is a contiguous float64 device tensor [B, p]")
    B, p = c.shape
    if not isinstance(W, torch.Tensor) or W.shape != c.shape or W.dtype != torch.float64 or not W.is_contiguous() or W.device != c.device:
        raise ValueError(f"{what}: W is a contiguous float64 tensor [B, p] on c's device")
    if not isinstance(sse, torch.Tensor) or sse.shape != (B,) or sse.dtype != torch.float64 or not sse.is_contiguous() or \
            sse.device != c.device:
        raise ValueError(f"{what}: sse is a contiguous float64 tensor [B] on c's device")
    bounds = np.ascontiguousarray(check_segments(bounds, p), dtype=np.int64)
    return B, p, bounds, len(bounds) - 1


def _dev_like(what, name, t, shape, c):
    import torch
    if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape or t.dtype != torch.float64 or not t.is_contiguous() or \
            t.device != c.device:
        raise ValueError(f"{what}: {name} is a contiguous float64 tensor {list(shape)} on c's device")


def log_evidence_dev(c, W, sse, n, bounds, s2, tau):
    """`qn_la_evidence` on device tensors: c, W `[B, p]`, sse `[B]`, s2 `[B, Hc]`, tau `[B, Hc, G]` float64 contiguous, bounds
    `[G + 1]` on the host -> `[B, Hc, 4 + 2 G]` float64 device tensor (the rows of `log_evidence`)."""
    import torch
    from . import _lib
    B, p, bounds, G = _dev_args("log_evidence_dev", c, W, sse, bounds)
    if not isinstance(s2, torch.Tensor) or s2.dim() != 2 or s2.shape[0] != B:
        raise ValueError("log_evidence_dev: s2 is a contiguous float64 tensor [B, Hc] on c's device")
    Hc = s2.shape[1]
    _dev_like("log_evidence_dev", "s2", s2, (B, Hc), c)
    _dev_like("log_evidence_dev", "tau", tau, (B, Hc, G), c)
    L = _lib.lib()
    need = int(L.qn_la_evidence_workspace_bytes(B, p, G, Hc))
    if need == 0:
        raise ValueError(L.qn_last_error().decode())
    out = torch.empty(B, Hc, _lib.EV_NOUT + 2 * G, dtype=torch.float64, device=c.device)
    ws = torch.empty(need // 8, dtype=torch.float64, device=c.device)
    with torch.cuda.device(c.device):
        _lib.check(L.qn_la_evidence(c.data_ptr(), W.data_ptr(), sse.data_ptr(), int(n), B, p, bounds.ctypes.data, G, Hc,
                                    s2.data_ptr(), tau.data_ptr(), out.data_ptr(), ws.data_ptr(), need, _lib.stream(c.device)),
                   "qn_la_evidence")
    return out


def tune_dev(c, W, sse, n, bounds, s2_0, tau_0, tol=DEFAULT_TOL, max_iter=DEFAULT_MAX_ITER, tune_noise=True, tune_prior=True,
             cov_scale=1.0, want_dinv=False, s2_min=DEFAULT_CLAMPS['s2_min'], s2_max=DEFAULT_CLAMPS['s2_max'],
             tau_min=DEFAULT_CLAMPS['tau_min'], tau_max=DEFAULT_CLAMPS['tau_max']):
    """`qn_la_tune` on device tensors: c, W `[B, p]`, sse, s2_0 `[B]`, tau_0 `[B, G]` float64 contiguous, one launch for all
    members -> a dict of float64 device tensors `s2` `[B]`, `tau` `[B, G]`, `rows` `[B, 4 + 2 G]`, `status` `[B, 6]` (`STATUS`)
    and, with want_dinv, `Dinv` and `Dih` `[B, p]` = 1 / (cov_scale lambda) and its root at the returned iterate."""
    import torch
    from . import _lib
    B, p, bounds, G = _dev_args("tune_dev", c, W, sse, bounds)
    _dev_like("tune_dev", "s2_0", s2_0, (B,), c)
    _dev_like("tune_dev", "tau_0", tau_0, (B, G), c)
    L = _lib.lib()
    need = int(L.qn_la_tune_workspace_bytes(B, p, G))
    if need == 0:
        raise ValueError(L.qn_last_error().decode())
    new = lambda *shape: torch.empty(*shape, dtype=torch.float64, device=c.device)      # noqa: E731
    res = dict(s2=new(B), tau=new(B, G), rows=new(B, _lib.EV_NOUT + 2 * G), status=new(B, _lib.EV_NSTATUS))
    if want_dinv:
        res.update(Dinv=new(B, p), Dih=new(B, p))
    ws = new(need // 8)
    with torch.cuda.device(c.device):
        _lib.check(L.qn_la_tune(c.data_ptr(), W.data_ptr(), sse.data_ptr(), int(n), B, p, bounds.ctypes.data, G, s2_0.data_ptr(),
                                tau_0.data_ptr(), float(tol), int(max_iter), float(s2_min), float(s2_max), float(tau_min),
                                float(tau_max), int(bool(tune_noise)), int(bool(tune_prior)), float(cov_scale),
                                res["s2"].data_ptr(), res["tau"].data_ptr(), res["rows"].data_ptr(), res["status"].data_ptr(),
                                res["Dinv"].data_ptr() if want_dinv else None, res["Dih"].data_ptr() if want_dinv else None,
                                ws.data_ptr(), need, _lib.stream(c.device)), "qn_la_tune")
    return res
