"""Isotropic Gaussian weight prior N(0, priorsigma^2 I) for `NN_MCMC` on every engine (build-only: the reference has no prior
there): the contract of qn_prior_fold (csrc/qn_prior.hip, include/quinn_amd.h), restated in numpy.

Every device engine funnels through a bare SSE and d SSE / d W, which its accept / leapfrog / adapt / swap / SG kernels turn
into log-posteriors and forces with gs = -0.5 / sigma^2.  The prior is written in exactly those units:

    lam  = sigma^2 / priorsigma^2
    c0   = sigma^2 * p * log(2 pi priorsigma^2)
    sse' = sse + lam |w|^2 + c0      ->  -0.5 sse' / sigma^2 - (N / 2) log 2 pi - N log sigma
                                          = loglik(w) + log N(w; 0, priorsigma^2 I), normaliser included
    g'   = g + 2 lam w               ->  -0.5 g' / sigma^2 = d loglik / dw - w / priorsigma^2

so one launch behind each forward / gradient call gives every existing kernel the prior.  A ladder's beta scales sse', prior
included (the constant cancels in the accept and the swap ratio): a hot rung's prior has variance priorsigma^2 / beta.  The
minibatch samplers rescale what they are given by n_rows / n_batch; `fold_constants` divides that out beforehand, so the prior
is exact and only the likelihood is estimated.

Not here: per-layer or ARD scales, hyper-priors, likelihood-only tempering.
"""
import numpy as np


def check_priorsigma(v):
    """None (no prior), or the prior's standard deviation as a float > 0; anything else raises ValueError."""
    if v is None:
        return None
    if isinstance(v, (bool, np.bool_, str, bytes)) or np.ndim(v) != 0:
        raise ValueError(f"priorsigma = {v!r}: None (no prior) or one finite standard deviation > 0")
    try:
        f = float(v)
    except (TypeError, ValueError):
        raise ValueError(f"priorsigma = {v!r}: None (no prior) or one finite standard deviation > 0") from None
    if not (f > 0.0 and np.isfinite(f)):
        raise ValueError(f"priorsigma = {v!r}: None (no prior) or one finite standard deviation > 0")
    return f


def fold_constants(sigma, priorsigma, p, n_rows=None, n_batch=None):
    """(lam, c0) of qn_prior_fold for the noise level sigma and p weights.  With a minibatch of n_batch of the n_rows data rows
    both are multiplied by n_batch / n_rows: qn_sg_step's (n_rows / n_batch) then leaves the prior unscaled."""
    sigma, ps = float(sigma), check_priorsigma(priorsigma)
    if ps is None:
        raise ValueError("fold_constants needs a priorsigma")
    lam = sigma * sigma / (ps * ps)
    c0 = sigma * sigma * int(p) * np.log(2.0 * np.pi * ps * ps)
    if n_batch is not None and n_rows is not None and int(n_batch) != int(n_rows):
        f = int(n_batch) / int(n_rows)
        lam, c0 = lam * f, c0 * f
    return float(lam), float(c0)


def fold(W, lam, c0, grad=None, sse=None):
    """The kernel's formulas on W [C, p] float64: (grad', sse') with grad' = grad + (2 lam) W in float64, rounded once to grad's
    dtype, and sse' = sse + (lam sum_j W^2 + c0); None stays None.  (The kernel's sum of squares has its own fixed order.)"""
    W = np.atleast_2d(np.asarray(W, dtype=np.float64))
    g2 = s2 = None
    if grad is not None:
        grad = np.asarray(grad)
        g2 = (grad.astype(np.float64) + (2.0 * lam) * W).astype(grad.dtype)
    if sse is not None:
        s2 = np.asarray(sse, dtype=np.float64) + (lam * np.sum(W * W, axis=-1) + c0)
    return g2, s2


def log_prior(W, priorsigma):
    """log N(w; 0, priorsigma^2 I) of every row of W [C, p] (normaliser included): float64 [C]."""
    ps = check_priorsigma(priorsigma)
    W = np.atleast_2d(np.asarray(W, dtype=np.float64))
    return -0.5 * np.sum(W * W, axis=-1) / ps ** 2 - 0.5 * W.shape[-1] * np.log(2.0 * np.pi * ps ** 2)


def grad_log_prior(W, priorsigma):
    """d log N(w; 0, priorsigma^2 I) / dw = -w / priorsigma^2, for every row of W [C, p]."""
    ps = check_priorsigma(priorsigma)
    return -np.atleast_2d(np.asarray(W, dtype=np.float64)) / ps ** 2
