"""Conjugate hyper-prior on the noise level `datanoise` for the device HMC / MALA engines (build-only: the reference's noise
level is a hand-set scalar), Gibbs-sampled on the device.  The contract of qn_noise_fold and qn_noise_gibbs (csrc/qn_prior.hip, csrc/qn_noise.hip,
include/quinn_amd.h) restated in numpy, and the authority for the draw.

One noise variance s2_c per chain, shared by all n = N * o entries of y (N rows, o outputs):

    y_k | w, s2 ~ N(M_w(x)_k, s2),      1 / s2 ~ Gamma(shape a0, rate b0),
    1 / s2 | w, y ~ Gamma(a0 + n / 2, rate b0 + SSE(w) / 2),      SSE(w) the data sum of squares alone, without the prior.

The weight prior is not scaled by s2: `priorsigma` and `hyperprior` keep their meaning.  The sampler alternates HMC / MALA steps
on w at fixed s2 with the exact Gibbs draw of s2.  The device kernels keep the NOMINAL sigma0 = datanoise they are called with
(h = 0.5 / sigma0^2 and the accept kernel's lik_const = (N / 2) log 2 pi + N log sigma0), so the noise level is written in those
units, per chain c:

    kappa[c] = sigma0^2 / s2_c
    d0[c]    = sigma0^2 (n log(2 pi s2_c) - 2 log p(s2_c) - N log(2 pi sigma0^2))
    log p(s2) = a0 log b0 - lgamma(a0) + (a0 + 1) log(1 / s2) - b0 / s2        (the density of s2, Jacobian included)
    sse' = (kappa sse + P) + d0,   P = sum_g lam_g S_g + c0 as `hyper.fold_g` adds it (absent without a weight prior)
    g'_j = kappa g_j + (2 lam_g(j)) w_j

and -(h sse' + lik_const) is the JOINT log density of (w, s2[, tau]) given the data (`log_joint`): what 'logpost', 'maxpost' and
the MAP bookkeeping of a run with a noise prior report.  The normaliser covers all N * o entries: the kernels' constant counts N,
d0 removes it.  `every` = 0 never draws: a fixed noise level `sigma_init` through the same fold; a0, b0 may then be omitted, and
the log p(s2) term of d0 is left out.

Not covered: per-output or heteroscedastic noise, any sampler but device HMC / MALA, ladders, graphs, RNet.
"""
import math

import numpy as np

from . import hyper

PURPOSE_NOISE = 12          # Philox purpose of the noise precision's Gamma variate (csrc/qn_mcmc_shared.h)
TWO_PI = 6.283185307179586
_KEYS = ('a0', 'b0', 'every', 'sigma_init')


def _pos(v, what):
    if isinstance(v, (bool, np.bool_, str, bytes)) or np.ndim(v) != 0:
        raise ValueError(f"noiseprior: {what} = {v!r} is one finite number > 0")
    try:
        f = float(v)
    except (TypeError, ValueError):
        raise ValueError(f"noiseprior: {what} = {v!r} is one finite number > 0") from None
    if not (f > 0.0 and np.isfinite(f)):
        raise ValueError(f"noiseprior: {what} = {v!r} is one finite number > 0")
    return f


def check_noiseprior(nprior):
    """None (the hand-set noise level), or the settings as a dict {a0, b0, every, sigma_init} with the defaults filled in
    (every=1, sigma_init=None: start at datanoise); anything else raises ValueError.  With every = 0 (never draw) a0 and b0 may
    be omitted -- both or neither; they are then None and the log p(s2) term of d0 is left out."""
    if nprior is None:
        return None
    if not isinstance(nprior, dict):
        raise ValueError(f"noiseprior = {nprior!r}: None or a dict(a0=, b0=, every=1, sigma_init=None)")
    unknown = sorted(set(nprior) - set(_KEYS))
    if unknown:
        raise ValueError(f"noiseprior: unknown keys {unknown} (known: {list(_KEYS)})")
    every = nprior.get('every', 1)
    if isinstance(every, (bool, np.bool_)) or not isinstance(every, (int, np.integer)) or every < 0:
        raise ValueError(f"noiseprior: every = {every!r} is an int >= 0 (a Gibbs round after every that many steps; 0: never)")
    out = {'a0': None, 'b0': None, 'every': int(every)}
    given = [k for k in ('a0', 'b0') if nprior.get(k) is not None]
    if every != 0 or given:
        for k in ('a0', 'b0'):
            if k not in given:
                raise ValueError(f"noiseprior needs {k} (1 / s2 ~ Gamma(shape a0, rate b0); only every = 0 runs without both)")
            out[k] = _pos(nprior[k], k)
    si = nprior.get('sigma_init')
    out['sigma_init'] = None if si is None else _pos(si, 'sigma_init')
    return out


def log_noiseprior(s2, a0, b0):
    """log p(s2), the density of the VARIANCE whose reciprocal is Gamma(shape a0, rate b0) (Jacobian included), elementwise --
    the kernel's expression."""
    s2 = np.asarray(s2, dtype=np.float64)
    kconst = a0 * math.log(b0) - math.lgamma(a0)
    return kconst + (a0 + 1.0) * np.log(1.0 / s2) - b0 / s2


def fold_constants_n(sigma0, s2, n, N, a0=None, b0=None):
    """(kappa [C], d0 [C]) of qn_noise_fold for the nominal noise level sigma0, the variances s2 [C], n = N * o entries of y in
    N rows; a0 = b0 = None leaves the log p(s2) term out (a fixed noise level)."""
    s2 = np.atleast_1d(np.asarray(s2, dtype=np.float64))
    s0sq = float(sigma0) * float(sigma0)
    nlog0 = float(N) * math.log(TWO_PI * s0sq)
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        data = float(n) * np.log(TWO_PI * s2)
        if a0 is not None:
            data = data - 2.0 * log_noiseprior(s2, float(a0), float(b0))
        return s0sq / s2, s0sq * (data - nlog0)


def fold_n(W, kappa, d0, lam=None, c0=None, seg=None, grad=None, sse=None):
    """The kernel's formulas on W [C, p] float64: (grad', sse') with grad' = kappa grad + (2 lam[c, g(j)]) W in float64 (one
    rounding per operation), rounded once to grad's dtype, and sse' = (kappa sse + P) + d0, P as `hyper.fold_g` adds it;
    lam = None: no weight prior (G = 0).  None stays None."""
    W = np.atleast_2d(np.asarray(W, dtype=np.float64))
    kappa, d0 = np.asarray(kappa, dtype=np.float64), np.asarray(d0, dtype=np.float64)
    g2 = s2 = None
    with np.errstate(invalid='ignore', over='ignore'):
        if grad is not None:
            grad = np.asarray(grad)
            g2 = kappa[:, None] * grad.astype(np.float64)
            if lam is not None:
                g2 = hyper.fold_g(W, lam, c0, seg, grad=g2)[0]
            g2 = g2.astype(grad.dtype)
        if sse is not None:
            s2 = kappa * np.asarray(sse, dtype=np.float64)
            if lam is not None:
                s2 = hyper.fold_g(W, lam, c0, seg, sse=s2)[1]
            s2 = s2 + d0
    return g2, s2


def lik_constants(sigma0, N):
    """(h, lik_const) of the sampler kernels at the nominal noise level: 0.5 / sigma0^2 and (N / 2) log 2 pi + N log sigma0."""
    sigma0 = float(sigma0)
    return 0.5 / (sigma0 * sigma0), 0.5 * N * math.log(2.0 * math.pi) + N * math.log(sigma0)


def _prior_term(cur, lam, c0, seg):
    """P [C] = sum_g lam_g S_g + c0 of the rows of cur, left to right (what `hyper.fold_g` adds to an SSE of 0); 0 without lam."""
    if lam is None:
        return 0.0
    lam = np.atleast_2d(np.asarray(lam, dtype=np.float64))
    return hyper._sum_lr(lam * hyper.group_sumsq(cur, seg)) + np.asarray(c0, dtype=np.float64)


def recover_sse(cur_lp, kappa, d0, sigma0, N, cur=None, lam=None, c0=None, seg=None):
    """The data SSE [C] of the states whose folded log density is cur_lp: the fold inverted in the kernel's order,
    F = (-cur_lp - lik_const) / h, sse = ((F - d0) - P) / kappa.  Cancellation bounds the error by a few
    eps ((|cur_lp| + |lik_const|) / h + |d0| + |P|) / kappa."""
    h, lik_const = lik_constants(sigma0, N)
    F = (-np.asarray(cur_lp, dtype=np.float64) - lik_const) / h
    sse = F - np.asarray(d0, dtype=np.float64)
    if lam is not None:
        sse = sse - _prior_term(np.atleast_2d(np.asarray(cur, dtype=np.float64)), lam, c0, seg)
    return sse / np.asarray(kappa, dtype=np.float64)


def gibbs_round(cur, grad_cur, cur_lp, kappa, d0, sigma0, n, N, a0, b0, seed, step, chain0=0, lam=None, c0=None, seg=None):
    """Everything one qn_noise_gibbs launch writes, from the state it reads: cur, grad_cur [C, p], cur_lp [C], the current kappa,
    d0 [C] and weight prior (lam [C, G], c0 [C], seg; None: G = 0); `step` is the step t just decided.  Returns {'s2', 'sigma',
    'kappa', 'd0', 'cur_lp', 'sse' [C], 'grad_cur' [C, p], 'ok' [C]}; a chain that is not `ok` (a recovered SSE that is not finite
    or negative, new constants that are not positive / finite) keeps everything ('s2' = sigma0^2 / kappa there)."""
    cur = np.atleast_2d(np.asarray(cur, dtype=np.float64))
    g = np.asarray(grad_cur, dtype=np.float64)
    kappa, d0, cur_lp = (np.asarray(v, dtype=np.float64) for v in (kappa, d0, cur_lp))
    C = cur.shape[0]
    s0sq = float(sigma0) * float(sigma0)
    h, _ = lik_constants(sigma0, N)
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        sse = recover_sse(cur_lp, kappa, d0, sigma0, N, cur, lam, c0, seg)
        fin = np.isfinite(sse) & (sse >= 0.0)
        prec = hyper.gamma_draw(seed, step, int(chain0) + np.arange(C), 0, float(a0) + 0.5 * float(n),
                                float(b0) + 0.5 * np.where(fin, sse, 0.0), purpose=PURPOSE_NOISE)
        s2n = np.where(fin, 1.0 / prec, np.nan)
        kn, d0n = fold_constants_n(sigma0, s2n, n, N, a0, b0)
        ok = fin & (kn > 0.0) & np.isfinite(kn) & (s2n > 0.0) & np.isfinite(s2n) & np.isfinite(d0n)
        rm1 = (kn / kappa - 1.0)[:, None]
        if lam is not None:
            t = np.repeat(2.0 * np.atleast_2d(np.asarray(lam, dtype=np.float64)), np.diff(np.asarray(seg, dtype=np.int64)), axis=-1) * cur
            gn = g + rm1 * (g - t)
        else:
            gn = g + rm1 * g
        nlp = cur_lp - h * ((kn - kappa) * sse + (d0n - d0))
    s2o = s0sq / kappa
    s2 = np.where(ok, s2n, s2o)
    return {'s2': s2, 'sigma': np.sqrt(s2), 'kappa': np.where(ok, kn, kappa), 'd0': np.where(ok, d0n, d0),
            'cur_lp': np.where(ok, nlp, cur_lp), 'sse': sse, 'grad_cur': np.where(ok[:, None], gn, g), 'ok': ok}


def log_joint(sse, s2, n, a0=None, b0=None, logprior=0.0):
    """log p(w, s2[, tau] | data) up to the evidence, float64 [C]: the Gaussian log-likelihood of all n entries of y at the
    variances s2 [C] from the data SSE [C], plus log p(s2) (left out with a0 = b0 = None), plus `logprior` (the weight prior's
    log density, with its hyper-prior if any: `prior.log_prior`, `hyper.log_joint` with loglik = 0) -- what 'logpost' of a run
    with a noise prior stores."""
    s2 = np.asarray(s2, dtype=np.float64)
    out = -0.5 * np.asarray(sse, dtype=np.float64) / s2 - 0.5 * float(n) * np.log(TWO_PI * s2)
    if a0 is not None:
        out = out + log_noiseprior(s2, float(a0), float(b0))
    return out + np.asarray(logprior, dtype=np.float64)
