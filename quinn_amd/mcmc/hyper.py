"""Hierarchical Gaussian weight prior for the device HMC / MALA engines (build-only: the reference has no prior in `NN_MCMC`):
per-group precisions with a conjugate Gamma hyper-prior, Gibbs-sampled on the device (Neal 1996).  The contract of
qn_prior_fold_g and qn_hyper_gibbs (csrc/qn_prior.hip, csrc/qn_hyper.hip, include/quinn_amd.h) restated in numpy, and the authority for the draw.

Groups g = 0 .. G - 1 (G <= 32) are contiguous segments [seg[g], seg[g + 1]) of the flat weight vector, n_g entries each:

    w_j | tau_g ~ N(0, 1 / tau_g)  (j in group g),      tau_g ~ Gamma(shape a0, rate b0),
    tau_g | w   ~ Gamma(a0 + n_g / 2, rate b0 + S_g / 2),      S_g = sum_{j in g} w_j^2.

The sampler alternates HMC / MALA steps on w at fixed tau with the exact Gibbs draw of tau.  The device kernels turn a bare SSE
and d SSE / d W into log-densities and forces with gs = -0.5 / sigma^2, so the prior is written in those units, per chain c:

    lam[c, g] = sigma^2 tau[c, g]
    c0[c]     = sigma^2 (sum_g n_g log(2 pi / tau[c, g]) - 2 log p(tau[c, :]))
    log p(tau) = sum_g (a0 log b0 - lgamma(a0) + (a0 - 1) log tau_g - b0 tau_g)
    sse' = sse + (sum_g lam[c, g] S_g + c0[c])          g'_j = g_j + (2 lam[c, g(j)]) w_j

and gs sse' + (likelihood constants) is the JOINT log density of (w, tau) given the data (`log_joint`).  That joint is what
'logpost', 'maxpost' and the MAP bookkeeping of a run with a hyper-prior report: it is a function of the chain's whole state, so
the R-hat of its trace means something.  A joint mode in tau is of limited use (the density of a precision near 0 or far out is
not where the posterior mass is): predict with `predict_ens` / `score`, not from the MAP.

`every` = 0 never draws: fixed per-group scales from `tau0`, the per-layer prior without a hyper-prior.

Not covered: ARD scales per input, any sampler but device HMC / MALA, ladders, graphs, RNet.
"""
import math

import numpy as np

from .sgmcmc import ctr_of, philox4x32

GMAX = 32                   # groups at most (the kernels keep the bounds and factors of every group in LDS)
PURPOSE_GAMMA = 11          # Philox purpose of the Gamma variates (csrc/qn_mcmc_shared.h)
GAMMA_TRIES = 64            # bound of the rejection loop; after it the draw is shape / rate
GROUPINGS = ('layer', 'tensor', 'all')
_KEYS = ('a0', 'b0', 'groups', 'every', 'tau0')


def _pos(v, what):
    if isinstance(v, (bool, np.bool_, str, bytes)) or np.ndim(v) != 0:
        raise ValueError(f"hyperprior: {what} = {v!r} is one finite number > 0")
    try:
        f = float(v)
    except (TypeError, ValueError):
        raise ValueError(f"hyperprior: {what} = {v!r} is one finite number > 0") from None
    if not (f > 0.0 and np.isfinite(f)):
        raise ValueError(f"hyperprior: {what} = {v!r} is one finite number > 0")
    return f


def check_hyperprior(hp):
    """None (no hyper-prior), or the settings as a dict {a0, b0, groups, every, tau0} with the defaults filled in (groups='layer',
    every=1, tau0=None); anything else raises ValueError.  tau0: None, one precision > 0 or a sequence of them (one per group:
    its length is checked against the groups by `initial_tau`)."""
    if hp is None:
        return None
    if not isinstance(hp, dict):
        raise ValueError(f"hyperprior = {hp!r}: None or a dict(a0=, b0=, groups='layer' | 'tensor' | 'all', every=1, tau0=None)")
    unknown = sorted(set(hp) - set(_KEYS))
    if unknown:
        raise ValueError(f"hyperprior: unknown keys {unknown} (known: {list(_KEYS)})")
    for k in ('a0', 'b0'):
        if k not in hp:
            raise ValueError(f"hyperprior needs {k} (tau_g ~ Gamma(shape a0, rate b0))")
    out = {'a0': _pos(hp['a0'], 'a0'), 'b0': _pos(hp['b0'], 'b0'), 'groups': hp.get('groups', 'layer')}
    if not isinstance(out['groups'], str) or out['groups'] not in GROUPINGS:
        raise ValueError(f"hyperprior: groups = {out['groups']!r} is 'layer', 'tensor' or 'all'")
    every = hp.get('every', 1)
    if isinstance(every, (bool, np.bool_)) or not isinstance(every, (int, np.integer)) or every < 0:
        raise ValueError(f"hyperprior: every = {every!r} is an int >= 0 (a Gibbs round after every that many steps; 0: never)")
    out['every'] = int(every)
    tau0 = hp.get('tau0')
    if tau0 is not None:
        if np.ndim(tau0) == 0:
            tau0 = _pos(tau0, 'tau0')
        else:
            if np.ndim(tau0) != 1 or len(tau0) < 1:
                raise ValueError(f"hyperprior: tau0 = {tau0!r} is one precision > 0 or one per group")
            tau0 = tuple(_pos(v, 'tau0[%d]' % i) for i, v in enumerate(tau0))
    elif out['every'] == 0:
        raise ValueError("hyperprior: every = 0 never draws the precisions, so it needs tau0 (the fixed per-group precisions)")
    out['tau0'] = tau0
    return out


def group_segments(arch, groups):
    """(seg int64 [G + 1], names) of the weight groups of an `MLPArch` in its flat layout [W_0, b_0, W_1, b_1, ...]:
    'layer' -- each Linear's weight and bias in one group; 'tensor' -- every parameter tensor its own group; 'all' -- one
    group.  More than 32 groups is a ValueError."""
    if groups not in GROUPINGS:
        raise ValueError(f"hyperprior: groups = {groups!r} is 'layer', 'tensor' or 'all'")
    if not hasattr(arch, 'dims') or not hasattr(arch, 'param_shapes') or type(arch).__name__ != 'MLPArch':
        raise ValueError(f"hyperprior: weight groups are defined for plain MLPs, not for {type(arch).__name__}")
    sizes = [int(np.prod(s)) for s in arch.param_shapes()]
    per = 2 if arch.bias else 1
    nlayer = len(arch.dims) - 1
    if groups == 'all':
        seg, names = [0, sum(sizes)], ['all']
    elif groups == 'tensor':
        seg = [0] + list(np.cumsum(sizes))
        names = [('W%d' if k % per == 0 else 'b%d') % (k // per) for k in range(len(sizes))]
    else:
        seg = [0] + [sum(sizes[:per * (k + 1)]) for k in range(nlayer)]
        names = ['layer%d' % k for k in range(nlayer)]
    if len(names) > GMAX:
        raise ValueError(f"hyperprior: groups = {groups!r} makes {len(names)} groups; at most {GMAX} are supported")
    return np.asarray(seg, dtype=np.int64), names


def check_segments(seg, p):
    """seg as int64 [G + 1] with seg[0] = 0, seg[G] = p, strictly increasing, 1 <= G <= 32; ValueError otherwise."""
    seg = np.asarray(seg)
    if seg.ndim != 1 or not 2 <= seg.size <= GMAX + 1 or not np.issubdtype(seg.dtype, np.integer):
        raise ValueError(f"seg = {seg!r}: G + 1 integer bounds, 1 <= G <= {GMAX}")
    seg = seg.astype(np.int64)
    if seg[0] != 0 or seg[-1] != int(p) or np.any(np.diff(seg) <= 0):
        raise ValueError(f"seg = {seg.tolist()}: seg[0] = 0, seg[G] = p = {p}, strictly increasing")
    return seg


def initial_tau(hp, G, priorsigma=None):
    """float64 [G]: tau0 (a scalar or G values) if given, else 1 / priorsigma^2 if priorsigma is, else the prior mean a0 / b0."""
    tau0 = hp['tau0']
    if tau0 is None:
        tau0 = 1.0 / float(priorsigma) ** 2 if priorsigma is not None else hp['a0'] / hp['b0']
    if np.ndim(tau0) == 0:
        return np.full(G, float(tau0))
    if len(tau0) != G:
        raise ValueError(f"hyperprior: tau0 has {len(tau0)} values for {G} groups")
    return np.asarray(tau0, dtype=np.float64)


def _c0_terms(tau, n, a0, b0):
    """[..., G]: n_g log(2 pi / tau_g) - 2 log p(tau_g), the kernel's expression."""
    kconst = a0 * math.log(b0) - math.lgamma(a0)
    return n * np.log(6.283185307179586 / tau) - 2.0 * (kconst + (a0 - 1.0) * np.log(tau) - b0 * tau)


def _sum_lr(x):
    """Sum over the last axis, left to right (the kernel's order)."""
    out = x[..., 0].copy()
    for g in range(1, x.shape[-1]):
        out = out + x[..., g]
    return out


def fold_constants_g(sigma, tau, seg, a0, b0):
    """(lam [C, G], c0 [C]) of qn_prior_fold_g for the noise level sigma and the precisions tau [C, G] (or [G])."""
    tau = np.atleast_2d(np.asarray(tau, dtype=np.float64))
    n = np.diff(np.asarray(seg, dtype=np.int64)).astype(np.float64)
    s2 = float(sigma) * float(sigma)
    return s2 * tau, s2 * _sum_lr(_c0_terms(tau, n, float(a0), float(b0)))


def group_sumsq(W, seg):
    """S [C, G]: the sum of squares of every group of every row of W [C, p]."""
    W = np.atleast_2d(np.asarray(W, dtype=np.float64))
    return np.stack([np.sum(W[:, lo:hi] ** 2, axis=-1) for lo, hi in zip(seg[:-1], seg[1:])], axis=-1)


def fold_g(W, lam, c0, seg, grad=None, sse=None):
    """The kernel's formulas on W [C, p] float64: (grad', sse') with grad' = grad + (2 lam[c, g(j)]) W in float64, rounded once
    to grad's dtype, and sse' = sse + (sum_g lam[c, g] S_g + c0[c]); None stays None."""
    W = np.atleast_2d(np.asarray(W, dtype=np.float64))
    lam = np.atleast_2d(np.asarray(lam, dtype=np.float64))
    rep = np.diff(np.asarray(seg, dtype=np.int64))
    g2 = s2 = None
    if grad is not None:
        grad = np.asarray(grad)
        g2 = (grad.astype(np.float64) + np.repeat(2.0 * lam, rep, axis=-1) * W).astype(grad.dtype)
    if sse is not None:
        s2 = np.asarray(sse, dtype=np.float64) + (_sum_lr(lam * group_sumsq(W, seg)) + np.asarray(c0, dtype=np.float64))
    return g2, s2


def u01(hi, lo):
    """The device's uniform in (0, 1) with 53 random bits from two Philox words."""
    bits = (np.asarray(hi, dtype=np.uint64) << np.uint64(21)) ^ (np.asarray(lo, dtype=np.uint64) >> np.uint64(11))
    return (bits.astype(np.float64) + 0.5) * (1.0 / 9007199254740992.0)


def gamma_draw(seed, step, chain, group, shape, rate, purpose=PURPOSE_GAMMA):
    """Gamma(shape, rate) variates by Marsaglia & Tsang (2000), the log test only, exactly as qn_hyper_gibbs draws them:
    Philox keyed (seed, 2 step + 1, [chain : 24][11 : 4][index : 36]) with index = (group << 16) | (attempt << 4) | block;
    block 0 of an attempt gives the normal (Box-Muller in float64 on u01(words 0, 1), u01(words 2, 3)), block 1 the uniform of
    the test; shape < 1 draws at shape + 1 and multiplies by u^(1 / shape), u from index (group << 16) | (64 << 4).  At most 64
    attempts, then shape / rate.  chain (GLOBAL id), group, shape and rate broadcast against each other.  `purpose`: the Philox
    purpose in the place of 11 (12: the noise level's round, `quinn_amd.mcmc.noise`)."""
    chain, group, shape, rate = np.broadcast_arrays(np.asarray(chain, dtype=np.uint64), np.asarray(group, dtype=np.uint64),
                                                    np.asarray(shape, dtype=np.float64), np.asarray(rate, dtype=np.float64))
    dims = shape.shape
    chain, group, shape, rate = chain.ravel(), group.ravel(), shape.ravel(), rate.ravel()
    stream = 2 * int(step) + 1
    small = shape < 1.0
    a = np.where(small, shape + 1.0, shape)
    d = a - 1.0 / 3.0
    c = 1.0 / np.sqrt(9.0 * d)
    out = shape / rate                                   # (what is left after the last attempt)
    gbits = group << np.uint64(16)
    todo = np.arange(shape.size)                         # the draws no attempt has accepted yet
    with np.errstate(invalid='ignore', divide='ignore'):
        for k in range(GAMMA_TRIES):
            if todo.size == 0:
                break
            idx = gbits[todo] | np.uint64(k << 4)
            b0 = philox4x32(seed, stream, ctr_of(chain[todo], purpose, idx))
            x = np.sqrt(-2.0 * np.log(u01(b0[:, 0], b0[:, 1]))) * np.cos(6.283185307179586 * u01(b0[:, 2], b0[:, 3]))
            t = 1.0 + c[todo] * x
            v = t * t * t
            b1 = philox4x32(seed, stream, ctr_of(chain[todo], purpose, idx | np.uint64(1)))
            dd = d[todo]
            acc = (t > 0.0) & (np.log(u01(b1[:, 0], b1[:, 1])) < 0.5 * x * x + dd - dd * v + dd * np.log(np.where(t > 0.0, v, 1.0)))
            hit = todo[acc]
            gam = (dd * v)[acc]
            sm = small[hit]
            if sm.any():
                bu = philox4x32(seed, stream, ctr_of(chain[hit], purpose, gbits[hit] | np.uint64(GAMMA_TRIES << 4)))
                gam = np.where(sm, gam * np.exp(np.log(u01(bu[:, 0], bu[:, 1])) / shape[hit]), gam)
            out[hit] = gam / rate[hit]
            todo = todo[~acc]
    return out.reshape(dims)


def gibbs_round(cur, grad_cur, cur_lp, lam, c0, seg, sigma, a0, b0, seed, step, chain0=0):
    """Everything one qn_hyper_gibbs launch writes, from the state it reads: cur, grad_cur [C, p], cur_lp [C], the current lam
    [C, G] and c0 [C]; `step` is the step t just decided.  Returns {'tau', 'lam' [C, G], 'c0', 'cur_lp' [C], 'grad_cur' [C, p],
    'ok' [C]}; a chain that is not `ok` (a non-finite S_g, or a new lam / c0 that is not positive / finite) keeps everything
    ('tau' = lam / sigma^2 there; the kernel repeats the chain's previous taus column)."""
    cur = np.atleast_2d(np.asarray(cur, dtype=np.float64))
    lam = np.atleast_2d(np.asarray(lam, dtype=np.float64))
    c0, cur_lp = np.asarray(c0, dtype=np.float64), np.asarray(cur_lp, dtype=np.float64)
    seg = np.asarray(seg, dtype=np.int64)
    C, G = lam.shape
    n = np.diff(seg).astype(np.float64)
    s2 = float(sigma) * float(sigma)
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        S = group_sumsq(cur, seg)
        fin = np.isfinite(S)
        tau = gamma_draw(seed, step, (int(chain0) + np.arange(C))[:, None], np.arange(G)[None, :], float(a0) + 0.5 * n[None, :],
                         float(b0) + 0.5 * np.where(fin, S, 0.0))
        tau = np.where(fin, tau, np.nan)
        lamn = s2 * tau
        term = _c0_terms(tau, n, float(a0), float(b0))
        ok = np.all((lamn > 0.0) & np.isfinite(lamn) & np.isfinite(term), axis=-1)
        c0n = s2 * _sum_lr(term)
        nlp = cur_lp + (-0.5 / s2) * (_sum_lr((lamn - lam) * S) + (c0n - c0))
        gn = np.asarray(grad_cur, dtype=np.float64) + np.repeat(2.0 * (lamn - lam), np.diff(seg), axis=-1) * cur
    k = ok[:, None]
    return {'tau': np.where(k, tau, lam / s2), 'lam': np.where(k, lamn, lam), 'c0': np.where(ok, c0n, c0),
            'cur_lp': np.where(ok, nlp, cur_lp), 'grad_cur': np.where(k, gn, np.asarray(grad_cur, dtype=np.float64)), 'ok': ok}


def log_prior_g(W, tau, seg):
    """log N(w; 0, diag(1 / tau_g(j))) of every row of W [C, p] for the precisions tau [C, G] (or [G]): float64 [C]."""
    tau = np.atleast_2d(np.asarray(tau, dtype=np.float64))
    n = np.diff(np.asarray(seg, dtype=np.int64)).astype(np.float64)
    return np.sum(-0.5 * tau * group_sumsq(W, seg) + 0.5 * n * np.log(tau / (2.0 * np.pi)), axis=-1)


def log_hyperprior(tau, a0, b0):
    """log p(tau) = sum_g log Gamma(tau_g; shape a0, rate b0) of every row of tau [C, G] (or [G]): float64 [C]."""
    tau = np.atleast_2d(np.asarray(tau, dtype=np.float64))
    return np.sum(a0 * math.log(b0) - math.lgamma(a0) + (a0 - 1.0) * np.log(tau) - b0 * tau, axis=-1)


def log_joint(W, tau, seg, a0, b0, loglik=0.0):
    """log p(w, tau | data) up to the evidence: loglik + log N(w; 0, 1 / tau) + log p(tau), float64 [C] -- what 'logpost' of a
    run with a hyper-prior stores (loglik: the log-likelihood of every row of W, e.g. `NN_MCMC.logpost_batch` without a prior)."""
    return np.asarray(loglik, dtype=np.float64) + log_prior_g(W, tau, seg) + log_hyperprior(tau, float(a0), float(b0))
