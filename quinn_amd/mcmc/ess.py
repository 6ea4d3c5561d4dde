"""Elliptical slice sampling (Murray, Adams & MacKay 2010) with asynchronous chain steps: the contract of the device engine
`DeviceESS` (qn_ess_begin / qn_ess_iter, csrc/qn_ess.hip; include/quinn_amd.h), restated in float64 numpy.

Target: pi(w) ~ L(w) N(w; 0, s^2 I) with log L = gs * sse(w) + const, gs = -0.5 / sigma^2 and s = priorsigma (`quinn_amd.mcmc.prior`).
The ellipse through the current point and a prior draw carries the prior, the slice test sees the likelihood alone: there is no
step size and nothing to warm up.  Per-chain state: the current point `cur`, the ellipse partner `nu`, the pending proposal
`prop`, the angle and its bracket (theta, tmin, tmax), the slice level logy, sse_cur and lp_cur, the chain's OWN step t, the
shrink count j of that step, and the counters ntrunc and nevals.

Start of step t (`ess_begin`; from cur, sse_cur):
    nu    = s z,  z ~ N(0, I): Philox block (seed, stream t, ctr_of(global chain, 7, column pair)) through the device's
            `normal2` -- the generator of the HMC momenta, float32 transcendentals, ~1e-6 relative accuracy, tails to 8 sigma.
            The restatement takes nu as an input (the tests feed the device's own)
    theta = 2 pi u01(w0, w1),  logy = gs sse_cur + log u01(w2, w3)      (w: the block (seed, t, ctr_of(chain, 8, 0)): `start_uniforms`)
    tmin  = theta - 2 pi,  tmax = theta,  j = 0,  prop = cur cos(theta) + nu sin(theta)

One iteration (`ess_iter`), given sse_prop of the pending proposal:
    accept iff sse_prop is finite and gs sse_prop > logy (a NaN comparison rejects):
        cur <- prop (a copy), sse_cur <- sse_prop, lp_cur = (gs sse_prop - const_lik) + (-0.5 |prop|^2 / s^2 - (p / 2) log(2 pi s^2)),
        row t + 1 of chain / lps / nev (= j + 1) written, best <- prop where lp_cur >= best_lp, t += 1 and, if t < nmcmc, the
        next step starts in the same iteration
    reject with j + 1 < max_shrink:  theta < 0 ? tmin = theta : tmax = theta;  theta = tmin + u (tmax - tmin) with u = u01(w0, w1)
        of the block (seed, t, ctr_of(chain, 8, j + 1)) (`shrink_uniform`);  j += 1;  prop = cur cos(theta) + nu sin(theta)
    reject with j + 1 == max_shrink (truncation): the chain stays -- row t + 1 repeats cur and lp_cur, nev = max_shrink,
        ntrunc += 1, t += 1 -- and starts its next step
    a done chain (t == nmcmc) is neither read nor written, in this and every later iteration
Every live chain's nevals grows by one per iteration: each forward evaluation is one some chain needs.

Truncation keeps the target: a step's transition is T(x, .) = A(x, .) + r(x) delta_x, where A collects the accepting paths.  The
untruncated kernel T_inf = A_inf + 0 satisfies detailed balance with pi (Murray et al. 2010, sec. 2.1: each accepting path and
its reverse have equal probability).  Truncating at max_shrink proposals keeps exactly the accepting paths of at most
max_shrink proposals, with the probabilities they have in the untruncated algorithm (a path's probability is a product over
its own proposals only), so A(x, dy) pi(dx) = A(y, dx) pi(dy) still holds path by path; the removed mass becomes the
self-transition r(x) delta_x, which is symmetric by itself.  Hence T is reversible with respect to pi for every max_shrink >= 1
(max_shrink = 1 is an independence-like move on a random ellipse), only slower to mix.  With max_shrink = 32 the bracket left at
truncation is about 2 pi / 2^32 in expectation.  That is rare on a broad likelihood and does happen on a narrow one (cfg2 with
sigma = 0.02, far from the mode: 1.4 % of the steps, profiles/ess.txt): watch `ntrunc` and raise max_shrink if it is not small.
"""
import math

import numpy as np

from .prior import check_priorsigma
from .sgmcmc import ctr_of, philox4x32

PURPOSE_NU, PURPOSE_ANGLE = 7, 8
TWO_PI = 2.0 * np.pi
ES_KEYS = ('theta', 'tmin', 'tmax', 'logy', 'sse_cur', 'lp_cur')      # es [2, C, 6] of the kernels, in this order
EI_KEYS = ('t', 'j', 'ntrunc', 'nevals')                              # ei [2, C, 4]


def u01(hi, lo):
    """The device's uniform in (0, 1) with 53 random bits from two Philox words (csrc/qn_mcmc_shared.h), bit for bit."""
    bits = (np.asarray(hi).astype(np.uint64) << np.uint64(21)) ^ (np.asarray(lo).astype(np.uint64) >> np.uint64(11))
    return (bits.astype(np.float64) + 0.5) * (1.0 / 9007199254740992.0)


def start_uniforms(seed, t, chain):
    """(u_theta, u_y) of GLOBAL chain `chain` (scalar or array) at the start of its step t: words (0, 1) and (2, 3) of the block
    (seed, stream t, ctr_of(chain, 8, 0))."""
    ch = np.asarray(chain, dtype=np.uint64)
    w = philox4x32(seed, int(t), ctr_of(ch, PURPOSE_ANGLE, np.zeros_like(ch)))
    return u01(w[..., 0], w[..., 1]), u01(w[..., 2], w[..., 3])


def shrink_uniform(seed, t, chain, j1):
    """The uniform that places the angle of shrink j1 = j + 1 >= 1 of step t: words (0, 1) of (seed, t, ctr_of(chain, 8, j1))."""
    ch = np.asarray(chain, dtype=np.uint64)
    w = philox4x32(seed, int(t), ctr_of(ch, PURPOSE_ANGLE, np.full_like(ch, int(j1))))
    return u01(w[..., 0], w[..., 1])


def lik_const(n_rows, sigma):
    """(N / 2) log 2 pi + N log sigma: log L(w) = gs sse(w) - lik_const (`DeviceEngine._const`)."""
    return (n_rows / 2) * np.log(2 * np.pi) + n_rows * np.log(float(sigma))


def log_post(sse, sq, p, n_rows, sigma, s):
    """Log-posterior with the prior from a point's SSE and its sum of squares sq = |w|^2, in the kernel's association."""
    gs = -0.5 / (float(sigma) * float(sigma))
    return (gs * np.asarray(sse, dtype=np.float64) - lik_const(n_rows, sigma)) + \
        (-0.5 / (float(s) * float(s)) * np.asarray(sq, dtype=np.float64) - 0.5 * int(p) * np.log(2.0 * np.pi * float(s) * float(s)))


def ellipse(cur, nu, theta):
    """cur cos(theta) + nu sin(theta)."""
    return np.asarray(cur, dtype=np.float64) * np.cos(theta) + np.asarray(nu, dtype=np.float64) * np.sin(theta)


def ess_begin(cur, sse_cur, nu, u_theta, u_y, sigma):
    """Start of a step of ONE chain from (cur [p], sse_cur) with the ellipse partner nu [p] (= s z) and the two uniforms of
    `start_uniforms`: dict(theta, tmin, tmax, logy, j = 0, prop)."""
    gs = -0.5 / (float(sigma) * float(sigma))
    theta = TWO_PI * float(u_theta)
    return {'theta': theta, 'tmin': theta - TWO_PI, 'tmax': theta, 'logy': gs * float(sse_cur) + np.log(float(u_y)), 'j': 0,
            'prop': ellipse(cur, nu, theta)}


def ess_iter(st, sse_prop, sigma, s, n_rows, nmcmc, max_shrink, u_shrink=None, nu_next=None, u_next=None, sq_prop=None):
    """One iteration of ONE chain.  st: dict with cur, nu, prop [p], theta, tmin, tmax, logy, sse_cur, lp_cur, t, j, ntrunc,
    nevals, best [p], best_lp (a new dict is returned, st is left alone).  sse_prop: the pending proposal's SSE.  u_shrink: the
    uniform of `shrink_uniform(seed, t, chain, j + 1)` (read on a shrink).  nu_next, u_next = (u_theta, u_y): the partner and
    the uniforms of step t + 1 (read when a next step starts).  sq_prop: |prop|^2 as the caller sums it (None: numpy's sum).
    Returns (state, event): event is 'done' | 'accept' | 'shrink' | 'trunc', and on 'accept' / 'trunc' the state carries
    'row' = (t + 1, chain row, lps entry, nev entry)."""
    st = {k: v for k, v in st.items() if k != 'row'}               # (arrays are replaced, never written in place)
    if st['t'] >= nmcmc:
        return st, 'done'
    gs = -0.5 / (float(sigma) * float(sigma))
    st['nevals'] += 1
    sse_prop = float(sse_prop)
    acc = bool(math.isfinite(sse_prop) and gs * sse_prop > float(st['logy']))
    if acc:
        sq = float(np.sum(st['prop'] * st['prop'])) if sq_prop is None else float(sq_prop)
        st['cur'] = st['prop']
        st['sse_cur'] = sse_prop
        st['lp_cur'] = float(log_post(sse_prop, sq, st['cur'].size, n_rows, sigma, s))
        st['row'] = (st['t'] + 1, st['cur'], st['lp_cur'], st['j'] + 1)
        if st['lp_cur'] >= st['best_lp']:
            st['best'], st['best_lp'] = st['cur'], st['lp_cur']
        event = 'accept'
    elif st['j'] + 1 < max_shrink:
        if st['theta'] < 0.0:
            st['tmin'] = st['theta']
        else:
            st['tmax'] = st['theta']
        st['theta'] = st['tmin'] + float(u_shrink) * (st['tmax'] - st['tmin'])
        st['j'] += 1
        st['prop'] = ellipse(st['cur'], st['nu'], st['theta'])
        return st, 'shrink'
    else:
        st['row'] = (st['t'] + 1, st['cur'], st['lp_cur'], int(max_shrink))
        st['ntrunc'] += 1
        event = 'trunc'
    st['t'] += 1
    if st['t'] < nmcmc:
        st['nu'] = np.array(nu_next, dtype=np.float64)
        st.update(ess_begin(st['cur'], st['sse_cur'], st['nu'], u_next[0], u_next[1], sigma))
    return st, event


def ess_chain(sse_fn, cur0, sigma, s, n_rows, nmcmc, max_shrink, rng):
    """One chain of nmcmc steps through `ess_begin` / `ess_iter` with host-drawn partners and uniforms (rng: a
    numpy RandomState; the device's streams are Philox): dict(chain [nmcmc + 1, p], lps, nev [nmcmc + 1], ntrunc, nevals).
    sse_fn: w [p] -> SSE."""
    cur = np.array(cur0, dtype=np.float64)
    p = cur.size
    sse0 = float(sse_fn(cur))
    lp0 = float(log_post(sse0, np.sum(cur * cur), p, n_rows, sigma, s))
    st = {'cur': cur, 'nu': float(s) * rng.standard_normal(p), 'sse_cur': sse0, 'lp_cur': lp0, 't': 0, 'ntrunc': 0, 'nevals': 0,
          'best': cur.copy(), 'best_lp': lp0}
    st.update(ess_begin(cur, sse0, st['nu'], rng.random_sample(), rng.random_sample(), sigma))
    chain, lps, nev = np.empty((nmcmc + 1, p)), np.empty(nmcmc + 1), np.zeros(nmcmc + 1, dtype=np.int32)
    chain[0], lps[0] = cur, lp0
    while st['t'] < nmcmc:
        st, event = ess_iter(st, sse_fn(st['prop']), sigma, s, n_rows, nmcmc, max_shrink, u_shrink=rng.random_sample(),
                             nu_next=float(s) * rng.standard_normal(p), u_next=(rng.random_sample(), rng.random_sample()))
        if event in ('accept', 'trunc'):
            r, row, lp, ne = st['row']
            chain[r], lps[r], nev[r] = row, lp, ne
    return {'chain': chain, 'lps': lps, 'nev': nev, 'ntrunc': st['ntrunc'], 'nevals': st['nevals'], 'best': st['best'],
            'best_lp': st['best_lp']}


def moment_deviation(samples, mean, cov):
    """(dm, dc) of pooled samples [n, p] against a Gaussian's mean and covariance, in units of the marginal standard
    deviations: dm = max_i |m_i - mean_i| / sd_i, dc = max_ij |S_ij - cov_ij| / (sd_i sd_j)."""
    x = np.asarray(samples, dtype=np.float64)
    sd = np.sqrt(np.diag(cov))
    dm = np.max(np.abs(x.mean(axis=0) - mean) / sd)
    dc = np.max(np.abs(np.cov(x.T) - cov) / np.outer(sd, sd))
    return float(dm), float(dc)


def gaussian_posterior(X, Y, sigma, s):
    """Closed-form posterior of the linear model y = X w + noise, noise ~ N(0, sigma^2), w ~ N(0, s^2 I): (mean [p], cov [p, p]).
    X [N, p] is the design matrix (a column of ones for a bias), Y [N] or [N, 1]."""
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    Y = np.asarray(Y, dtype=np.float64).reshape(X.shape[0])
    prec = X.T @ X / float(sigma) ** 2 + np.eye(X.shape[1]) / float(s) ** 2
    cov = np.linalg.inv(prec)
    return cov @ (X.T @ Y) / float(sigma) ** 2, cov


def check_ess_args(priorsigma, max_shrink=32, block=32):
    """Refuses what the sampler cannot run; returns (priorsigma, max_shrink, block) as float, int, int."""
    if priorsigma is None:
        raise ValueError("priorsigma = None: elliptical slice sampling needs the Gaussian weight prior N(0, priorsigma^2 I); "
                         "pass priorsigma > 0")
    ps = check_priorsigma(priorsigma)
    for name, v in (('max_shrink', max_shrink), ('block', block)):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or int(v) < 1:
            raise ValueError(f"{name} = {v!r}: an integer >= 1")
    if int(max_shrink) > 2 ** 31 - 1 or int(block) > 2 ** 20:
        raise ValueError(f"max_shrink = {max_shrink!r} / block = {block!r}: too large")
    return ps, int(max_shrink), int(block)
