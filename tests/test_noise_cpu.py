"""CPU: the contract of the noise prior in numpy (`quinn_amd.mcmc.noise`) -- the refusals of `check_noiseprior`, the fold
constants against a direct evaluation of the joint density, the inversion of the fold within its cancellation bound, a Gibbs
sampler built from `noise.gibbs_round` against the exact marginal of a conjugate toy model -- and which launches
`DeviceHMC._step` and the step after it make when the run state holds a noise level, recorded on stub objects in the style of
test_hyper_calls_cpu.py.  No device is needed."""
import math
import os

import numpy as np
import pytest

from quinn_amd import _lib
from quinn_amd.mcmc import hyper as hy
from quinn_amd.mcmc import noise as nz
from quinn_amd.mcmc.device_hmc import DeviceHMC

EPS = 2.0 ** -52


def test_check_noiseprior_fills_defaults_and_refuses_the_rest():
    assert nz.check_noiseprior(None) is None
    assert nz.check_noiseprior(dict(a0=3, b0=1)) == dict(a0=3.0, b0=1.0, every=1, sigma_init=None)
    assert nz.check_noiseprior(dict(a0=2.5, b0=0.5, every=4, sigma_init=0.1)) == dict(a0=2.5, b0=0.5, every=4, sigma_init=0.1)
    assert nz.check_noiseprior(dict(every=0, sigma_init=0.2)) == dict(a0=None, b0=None, every=0, sigma_init=0.2)
    assert nz.check_noiseprior(dict(every=0)) == dict(a0=None, b0=None, every=0, sigma_init=None)
    assert nz.check_noiseprior(dict(a0=3, b0=1, every=0))['a0'] == 3.0
    done = nz.check_noiseprior(dict(a0=3, b0=1))
    assert nz.check_noiseprior(done) == done                                  # the filled-in dict passes again (engine clones)
    for bad in ("gamma", 3.0, [3, 1], dict(a0=3), dict(b0=1), dict(), dict(a0=3, b0=1, every=-1), dict(a0=3, b0=1, every=1.5),
                dict(a0=3, b0=1, every=True), dict(a0=0.0, b0=1), dict(a0=3, b0=-1.0), dict(a0=np.inf, b0=1),
                dict(a0=3, b0=np.nan), dict(a0="3", b0=1), dict(a0=[3.0], b0=1), dict(a0=3, b0=1, sigma_init=0.0),
                dict(a0=3, b0=1, sigma_init=-0.1), dict(a0=3, b0=1, sigma_init=np.inf), dict(a0=3, b0=1, sigma=0.1),
                dict(a0=3, every=0), dict(b0=1, every=0)):
        with pytest.raises(ValueError, match="noiseprior"):
            nz.check_noiseprior(bad)


def _log_joint_direct(sse, s2, n, a0, b0):
    """log N(y; f, s2 I_n) + log p(s2) written out with math only: 1 / s2 ~ Gamma(a0, rate b0), the Jacobian 1 / s2^2."""
    loglik = -0.5 * sse / s2 - 0.5 * n * math.log(2.0 * math.pi * s2)
    prec = 1.0 / s2
    log_gamma_prec = a0 * math.log(b0) - math.lgamma(a0) + (a0 - 1.0) * math.log(prec) - b0 * prec
    return loglik + log_gamma_prec + 2.0 * math.log(prec)


@pytest.mark.parametrize("N,o", [(8, 1), (8, 3), (48, 2)])
def test_fold_constants_give_the_joint_density_in_the_kernels_units(N, o):
    sigma0, a0, b0, n = 0.3, 3.0, 1.5, N * o
    rs = np.random.RandomState(N + o)
    s2 = np.exp(rs.randn(5))
    sse = 5.0 + 40.0 * rs.rand(5)
    kappa, d0 = nz.fold_constants_n(sigma0, s2, n, N, a0, b0)
    assert np.array_equal(kappa, sigma0 * sigma0 / s2)
    h, lik_const = nz.lik_constants(sigma0, N)
    got = -(h * nz.fold_n(np.zeros((5, 2)), kappa, d0, sse=sse)[1] + lik_const)
    want = np.array([_log_joint_direct(sse[c], s2[c], n, a0, b0) for c in range(5)])
    np.testing.assert_allclose(got, want, rtol=1e-13, atol=1e-12)
    np.testing.assert_allclose(nz.log_joint(sse, s2, n, a0, b0), want, rtol=1e-13, atol=1e-12)
    # a fixed level (no a0, b0): the likelihood alone; and at s2 = sigma0^2 with o = 1 the fold is the identity
    k1, d1 = nz.fold_constants_n(sigma0, s2, n, N)
    got = -(h * nz.fold_n(np.zeros((5, 2)), k1, d1, sse=sse)[1] + lik_const)
    np.testing.assert_allclose(got, -0.5 * sse / s2 - 0.5 * n * np.log(2 * np.pi * s2), rtol=1e-13, atol=1e-12)
    if o == 1:
        k1, d1 = nz.fold_constants_n(sigma0, np.full(5, sigma0 * sigma0), n, N)
        assert np.all(k1 == 1.0) and np.all(d1 == 0.0)


def test_fold_n_is_the_scaled_likelihood_plus_the_prior_fold():
    C, p, seg = 3, 37, np.array([0, 5, 6, 30, 37])
    rs = np.random.RandomState(3)
    W, g, sse = rs.randn(C, p), 3.0 * rs.randn(C, p), 10.0 + rs.rand(C)
    lam, c0, kappa, d0 = 0.2 + rs.rand(C, 4), rs.randn(C), 0.5 + rs.rand(C), rs.randn(C)
    g2, s2 = nz.fold_n(W, kappa, d0, lam, c0, seg, grad=g, sse=sse)
    assert np.array_equal(g2, kappa[:, None] * g + np.repeat(2.0 * lam, np.diff(seg), axis=1) * W)
    np.testing.assert_allclose(s2, kappa * sse + (lam * hy.group_sumsq(W, seg)).sum(axis=1) + c0 + d0, rtol=1e-14)
    # kappa = 1, d0 = 0: hyper.fold_g bit for bit, float64 and float32
    one, zero = np.ones(C), np.zeros(C)
    for gg in (g, g.astype(np.float32)):
        a, b = nz.fold_n(W, one, zero, lam, c0, seg, grad=gg, sse=sse), hy.fold_g(W, lam, c0, seg, grad=gg, sse=sse)
        assert a[0].dtype == gg.dtype and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    # no weight prior
    g0, s0 = nz.fold_n(W, kappa, d0, grad=g, sse=sse)
    assert np.array_equal(g0, kappa[:, None] * g) and np.array_equal(s0, kappa * sse + d0)
    assert nz.fold_n(W, kappa, d0) == (None, None)


@pytest.mark.parametrize("with_prior", [False, True])
def test_recover_sse_inverts_the_fold_within_the_cancellation_bound(with_prior):
    C, p, seg, N, o, sigma0, a0, b0 = 6, 37, np.array([0, 5, 6, 30, 37]), 16, 2, 0.3, 3.0, 1.5
    rs = np.random.RandomState(11)
    W, sse = rs.randn(C, p), 2.0 + 30.0 * rs.rand(C)
    kappa, d0 = nz.fold_constants_n(sigma0, np.exp(0.5 * rs.randn(C)) * 0.1, N * o, N, a0, b0)
    lam = c0 = sg = None
    P = np.zeros(C)
    if with_prior:
        lam, c0 = hy.fold_constants_g(sigma0, 0.5 + rs.rand(C, 4), seg, 2.0, 1.5)
        sg = seg
        P = nz._prior_term(W, lam, c0, seg)
    h, lik_const = nz.lik_constants(sigma0, N)
    cur_lp = -(h * nz.fold_n(W, kappa, d0, lam, c0, sg, sse=sse)[1] + lik_const)
    got = nz.recover_sse(cur_lp, kappa, d0, sigma0, N, W, lam, c0, sg)
    bound = 16 * EPS * ((np.abs(cur_lp) + abs(lik_const)) / h + np.abs(d0) + np.abs(P)) / kappa
    print("recovered SSE: error", np.abs(got - sse), "bound", bound)
    assert np.all(np.abs(got - sse) <= bound) and np.all(bound < 1e-9 * sse)


def _marginal_moments(y, a0, b0):
    """(E[1 / s2], E[s2]) of p(s2 | y) for y_k ~ N(mu, s2), mu ~ N(0, 1), 1 / s2 ~ Gamma(a0, rate b0): mu integrated out in
    closed form (y ~ N(0, s2 I + 1 1^T)), s2 by the trapezoid rule on a fine grid of u = log s2."""
    n, sy, syy = len(y), float(np.sum(y)), float(np.sum(y * y))
    u = np.linspace(-12.0, 12.0, 200001)
    s2 = np.exp(u)
    logp = -0.5 * ((n - 1) * u + np.log(s2 + n)) - 0.5 * (syy - sy * sy / (s2 + n)) / s2 \
        + (a0 + 1.0) * np.log(1.0 / s2) - b0 / s2 + u                         # (+ u: the Jacobian of s2 = exp(u))
    w = np.exp(logp - logp.max())

    def trapezoid(f):
        return float(np.sum(0.5 * (f[1:] + f[:-1]) * np.diff(u)))
    z = trapezoid(w)
    return trapezoid(w / s2) / z, trapezoid(w * s2) / z


def test_the_contract_samples_the_model():
    """A Gibbs sampler whose s2 update IS `noise.gibbs_round` (the state of a one-weight 'network' w = mu, p = 1, whose data SSE is
    sum (y_k - mu)^2, folded into cur_lp as the engine folds it) and whose mu update is the exact Gaussian conditional; 64
    independent chains, 400 sweeps, 50 burned.  The chains' time averages of 1 / s2 and s2 against the marginal by quadrature,
    within 5 standard errors over chains."""
    n, a0, b0, sigma0, C, T, burn = 8, 3.0, 1.0, 0.7, 64, 400, 50
    rs = np.random.RandomState(5)
    y = 0.4 + 0.8 * rs.randn(n)
    h, lik_const = nz.lik_constants(sigma0, n)
    mu = rs.randn(C)
    kappa, d0 = nz.fold_constants_n(sigma0, np.full(C, sigma0 * sigma0), n, n, a0, b0)
    trace = np.empty((C, T))
    for t in range(T):
        s2 = sigma0 * sigma0 / kappa
        v = 1.0 / (1.0 + n / s2)
        mu = v * y.sum() / s2 + np.sqrt(v) * rs.randn(C)
        sse = ((y[None, :] - mu[:, None]) ** 2).sum(axis=1)
        cur_lp = -(h * nz.fold_n(mu[:, None], kappa, d0, sse=sse)[1] + lik_const)
        r = nz.gibbs_round(mu[:, None], np.zeros((C, 1)), cur_lp, kappa, d0, sigma0, n, n, a0, b0, seed=17, step=t, chain0=3)
        assert r['ok'].all()
        np.testing.assert_allclose(r['sse'], sse, rtol=1e-9)
        kappa, d0 = r['kappa'], r['d0']
        trace[:, t] = r['s2']
    want_prec, want_s2 = _marginal_moments(y, a0, b0)
    for per_chain, exact, what in (((1.0 / trace[:, burn:]).mean(axis=1), want_prec, "E[1 / s2]"),
                                   (trace[:, burn:].mean(axis=1), want_s2, "E[s2]")):
        mean, se = per_chain.mean(), per_chain.std(ddof=1) / np.sqrt(C)
        print(what, "exact", exact, "mean", mean, "z", (mean - exact) / se)
        assert abs(mean - exact) <= 5 * se, (what, mean, exact, se)


def test_gibbs_round_refreshes_the_cached_state_consistently():
    """After a round, cur_lp and grad_cur are those of a fresh fold at the new constants (to rounding), with and without a
    weight prior; a chain whose recovered SSE is NaN or negative keeps everything."""
    C, p, seg, N, o, sigma0, a0, b0 = 4, 37, np.array([0, 5, 6, 30, 37]), 16, 2, 0.3, 3.0, 1.5
    rs = np.random.RandomState(2)
    W, g, sse = rs.randn(C, p), 3.0 * rs.randn(C, p), 2.0 + 30.0 * rs.rand(C)
    kappa, d0 = nz.fold_constants_n(sigma0, np.full(C, 0.05), N * o, N, a0, b0)
    h, lik_const = nz.lik_constants(sigma0, N)
    for lam, c0, sg in ((None, None, None), hy.fold_constants_g(sigma0, 0.5 + rs.rand(C, 4), seg, 2.0, 1.5) + (seg,)):
        gcur, s1 = nz.fold_n(W, kappa, d0, lam, c0, sg, grad=g, sse=sse)
        cur_lp = -(h * s1 + lik_const)
        r = nz.gibbs_round(W, gcur, cur_lp, kappa, d0, sigma0, N * o, N, a0, b0, 9, 4, 2, lam, c0, sg)
        assert r['ok'].all() and not np.any(r['kappa'] == kappa)
        k2, d2 = nz.fold_constants_n(sigma0, r['s2'], N * o, N, a0, b0)
        assert np.array_equal(k2, r['kappa']) and np.array_equal(d2, r['d0']) and np.array_equal(r['sigma'], np.sqrt(r['s2']))
        g2, s2_ = nz.fold_n(W, k2, d2, lam, c0, sg, grad=g, sse=sse)
        np.testing.assert_allclose(r['grad_cur'], g2, rtol=1e-11, atol=1e-12)
        np.testing.assert_allclose(r['cur_lp'], -(h * s2_ + lik_const), rtol=1e-11)
        # the draw is keyed by the GLOBAL chain id
        one = nz.gibbs_round(W[2:3], gcur[2:3], cur_lp[2:3], kappa[2:3], d0[2:3], sigma0, N * o, N, a0, b0, 9, 4, 4,
                             None if lam is None else lam[2:3], None if c0 is None else c0[2:3], sg)
        assert one['s2'][0] == r['s2'][2]
        bad_lp = cur_lp.copy()
        bad_lp[1], bad_lp[3] = np.nan, 1e9                                     # NaN; an SSE far below zero
        b = nz.gibbs_round(W, gcur, bad_lp, kappa, d0, sigma0, N * o, N, a0, b0, 9, 4, 2, lam, c0, sg)
        assert list(b['ok']) == [True, False, True, False]
        for c in (1, 3):
            assert b['kappa'][c] == kappa[c] and b['d0'][c] == d0[c] and np.array_equal(b['grad_cur'][c], gcur[c])
            assert np.array_equal(b['cur_lp'][c], bad_lp[c], equal_nan=True) and b['s2'][c] == sigma0 ** 2 / kappa[c]
        for c in (0, 2):
            assert b['s2'][c] == r['s2'][c] and b['cur_lp'][c] == r['cur_lp'][c]


def test_the_header_declares_the_two_entry_points_and_the_build_compiles_them():
    fold, gibbs = _lib.FUNCTIONS['qn_noise_fold'], _lib.FUNCTIONS['qn_noise_gibbs']
    assert len(fold[1]) == 14 and len(gibbs[1]) == 29 and len(_lib.FUNCTIONS) == 72
    assert 'qn_noise.hip' in _lib.SOURCES and os.path.exists(os.path.join(_lib.CSRC, 'qn_noise.hip'))
    assert nz.PURPOSE_NOISE == 12 and hy.PURPOSE_GAMMA == 11
    # purpose 12 is a stream of its own: the same key under purpose 11 gives another variate
    a = hy.gamma_draw(1, 2, 3, 0, 4.0, 2.0, purpose=nz.PURPOSE_NOISE)
    assert a != hy.gamma_draw(1, 2, 3, 0, 4.0, 2.0) and a == hy.gamma_draw(1, 2, 3, 0, 4.0, 2.0, purpose=12)


# ------------------------------------------------------------------------------------------------ recorded launches
SIGMA, EPSILON, CHAIN0, SEED, NMCMC, N_ROWS, QDT, C, P, STREAM = 0.25, 0.0125, 6, 991, 40, 48, 1, 4, 97, "stream"
NAMES = ["qn_hmc_begin", "qn_hmc_leap", "qn_hmc_accept", "qn_hmc_begin_s", "qn_hmc_leap_s", "qn_hmc_adapt"]
PRIOR = (0.37, -1.25)


class _T:
    """Stands for a device tensor: an address and a shape; indexing gives the slot's address."""

    def __init__(self, addr):
        self.addr, self.shape = addr, (C, P)

    def data_ptr(self):
        return self.addr

    def __getitem__(self, k):
        return _T(self.addr + 0x100 * (k + 1))


class _Lib:
    def __init__(self, calls):
        for n in NAMES:
            setattr(self, n, lambda *a, _n=n: calls.append((_n, a)) or 0)


def _addr(v):
    return v.addr if isinstance(v, _T) else v


class _Op:
    qdt, N = QDT, N_ROWS

    def __init__(self, calls):
        self.calls = calls

    def sse_grad(self, q, out):
        self.calls.append(("sse_grad", (q.addr, out[0].addr, out[1].addr)))

    def prior_fold(self, W, lam, c0, sse=None, grad=None):
        self.calls.append(("prior_fold", (W.addr, lam, c0, sse.addr, grad.addr)))

    def prior_fold_g(self, W, lam, c0, seg, sse=None, grad=None):
        self.calls.append(("prior_fold_g", (W.addr, lam.addr, c0.addr, seg.addr, sse.addr, grad.addr)))

    def noise_fold(self, W, kappa, d0, lam=None, c0=None, seg=None, sse=None, grad=None):
        self.calls.append(("noise_fold", tuple(_addr(v) for v in (W, kappa, d0, lam, c0, seg, sse, grad))))

    def hyper_gibbs(self, *a):
        self.calls.append(("hyper_gibbs", tuple(_addr(v) for v in a)))

    def noise_gibbs(self, *a):
        self.calls.append(("noise_gibbs", tuple(_addr(v) for v in a)))


class _Engine(DeviceHMC):
    def _stream(self):
        return STREAM


def _engine(L_, prior=None):
    calls = []
    e = _Engine.__new__(_Engine)
    e.sigma, e.epsilon, e.L, e.chain0, e.seed, e._prior, e.target_accept = SIGMA, EPSILON, L_, CHAIN0, SEED, prior, 0.8
    e._L, e.op = _Lib(calls), _Op(calls)
    return e, calls


KEYS = ['cur', 'gcur', 'mom', 'q', 'gq', 'sse', 'kcur', 'kprop', 'cur_lp', 'best', 'best_lp', 'chain', 'lps', 'alphas', 'nacc',
        'step', 'eps', 'scale', 'lam', 'c0', 'seg', 'taus', 'kappa', 'd0', 'sig', 'plam', 'pc0', 'pseg']
A = {k: 0x10000 * (i + 1) for i, k in enumerate(KEYS)}


def _state(par, **extra):
    s = {k: _T(A[k]) for k in KEYS[:16]}
    s.update(par=par, qc=None, g64=None)
    s.update({k: (None if v is None else _T(A[k])) for k, v in extra.items()})
    return s


@pytest.mark.parametrize("prior", [None, PRIOR])
@pytest.mark.parametrize("kind", ["none", "scalar", "hyper"])
@pytest.mark.parametrize("npar", [0, 1])
@pytest.mark.parametrize("L_", [1, 3])
@pytest.mark.parametrize("adapt", [False, True])
def test_with_kappa_set_the_step_makes_one_noise_fold_and_never_a_prior_fold(prior, kind, npar, L_, adapt):
    e, calls = _engine(L_, prior)
    extra = dict(kappa=1, d0=1, sig=1, **(dict(eps=1, scale=1) if adapt else {}))
    if kind == "scalar":
        extra.update(plam=1, pc0=1, pseg=1)
    if kind == "hyper":
        extra.update(lam=1, c0=1, seg=1, taus=1)
    s = _state(1, **extra)
    s.update(npar=npar, nround=2, noise=(3.0, 1.0, 96), hpar=1, hround=3, hyper=(3.0, 2.0))
    e._step(s, NMCMC)
    sfx = "_s" if adapt else ""
    assert [n for n, _ in calls] == ["qn_hmc_begin" + sfx] + ["sse_grad", "noise_fold", "qn_hmc_leap" + sfx] * L_ + ["qn_hmc_accept"]
    slot = 0x100 * (npar + 1)                                                 # kappa[npar], d0[npar]: the current slot
    wprior = {"none": (None, None, None), "scalar": (A['plam'], A['pc0'], A['pseg']),
              "hyper": (A['lam'] + 0x200, A['c0'] + 0x200, A['seg'])}[kind]     # (lam[hpar = 1], c0[hpar = 1])
    assert all(a == (A['q'], A['kappa'] + slot, A['d0'] + slot) + wprior + (A['sse'], A['gq']) for n, a in calls if n == "noise_fold")
    assert s['par'] == 0 and s['npar'] == npar and s['nround'] == 2          # a step flips the step parity only


@pytest.mark.parametrize("L_", [1, 3])
def test_without_kappa_the_recorded_sequence_is_the_one_recorded_today(L_):
    for prior, fold in ((None, []), (PRIOR, ["prior_fold"])):
        for extra in (dict(), dict(kappa=None), dict(lam=None, kappa=None)):
            e, calls = _engine(L_, prior)
            s = _state(1, **extra)
            e._step(s, NMCMC)
            assert [n for n, _ in calls] == ["qn_hmc_begin"] + ["sse_grad"] + fold + ["qn_hmc_leap"] + \
                (["sse_grad"] + fold + ["qn_hmc_leap"]) * (L_ - 1) + ["qn_hmc_accept"]
            assert all(a == (A['q'],) + PRIOR + (A['sse'], A['gq']) for n, a in calls if n == "prior_fold")
            assert calls[-1][1] == (A['q'], A['gq'], A['sse'], A['kcur'], A['kprop'], SIGMA, N_ROWS, C, CHAIN0, P, NMCMC, SEED,
                                    A['cur'], A['gcur'], A['cur_lp'], A['best'], A['best_lp'], A['chain'], A['lps'], A['alphas'],
                                    A['nacc'], A['step'], 1, STREAM)
    # a hyper-prior alone: the per-group fold, as before
    e, calls = _engine(L_, PRIOR)
    s = _state(1, lam=1, c0=1, seg=1, taus=1)
    s.update(hpar=0, hround=0, hyper=(3.0, 2.0))
    e._step(s, NMCMC)
    assert [n for n, _ in calls] == ["qn_hmc_begin"] + ["sse_grad", "prior_fold_g", "qn_hmc_leap"] * L_ + ["qn_hmc_accept"]


@pytest.mark.parametrize("par,npar", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("kind", ["none", "scalar", "hyper"])
def test_the_noise_round_gets_the_state_both_parities_and_the_round_and_flips_them(par, npar, kind):
    e, calls = _engine(1)
    extra = dict(kappa=1, d0=1, sig=1)
    if kind == "scalar":
        extra.update(plam=1, pc0=1, pseg=1)
    if kind == "hyper":
        extra.update(lam=1, c0=1, seg=1, taus=1)
    s = _state(par, **extra)
    s.update(npar=npar, nround=2, noise=(3.0, 1.0, 96), hpar=0, hround=3, hyper=(3.0, 2.0))
    e._noise_step(s, NMCMC)
    wprior = {"none": (None, None, None), "scalar": (A['plam'], A['pc0'], A['pseg']),
              "hyper": (A['lam'] + 0x100, A['c0'] + 0x100, A['seg'])}[kind]     # (the slot hpar = 0: current after the hyper round)
    assert calls == [("noise_gibbs", (A['cur'], A['gcur'], A['cur_lp'], A['best_lp'], A['lps'], A['kappa'], A['d0']) + wprior +
                      (A['sig'], A['step'], SIGMA, 3.0, 1.0, 96, 2, CHAIN0, SEED, par, npar))]
    assert (s['par'], s['npar'], s['nround']) == (1 - par, 1 - npar, 3)


def test_the_order_after_a_step_is_accept_adapt_hyper_round_noise_round():
    """`_gibbs_step`, the step `_run_gen` takes under a hyper-prior and / or a noise prior: the noise round reads the slot of
    lam / c0 the hyper round has just made current; a round is skipped when its `every` does not divide the step count."""
    e, calls = _engine(1)
    s = _state(0, kappa=1, d0=1, sig=1, lam=1, c0=1, seg=1, taus=1, eps=1, scale=1)
    s.update(npar=0, nround=0, noise=(3.0, 1.0, 96), hpar=0, hround=0, hyper=(3.0, 2.0), da=_T(1), wmean=None, wm2=None)
    s.update(nstep=0, hevery=1, nevery=1)
    e._gibbs_step(s, NMCMC, dict(m=1, collect=False, finish=False, freeze=False, n=0))
    assert [n for n, _ in calls] == ["qn_hmc_begin_s", "sse_grad", "noise_fold", "qn_hmc_leap_s", "qn_hmc_accept", "qn_hmc_adapt",
                                     "hyper_gibbs", "noise_gibbs"]
    hyper_call, noise_call = calls[-2][1], calls[-1][1]
    assert hyper_call[-2:] == (1, 0) and noise_call[-2:] == (0, 0)              # step parity 1 -> 0 -> 1; own parities 0
    assert noise_call[7:10] == (A['lam'] + 0x200, A['c0'] + 0x200, A['seg'])  # lam[1]: written by the hyper round
    assert (s['par'], s['hpar'], s['npar'], s['hround'], s['nround']) == (1, 1, 1, 1, 1)
    del calls[:]
    s.update(hevery=0, nevery=2)                                             # step 2: no hyper round, a noise round; step 3: neither
    e._gibbs_step(s, NMCMC)
    e._gibbs_step(s, NMCMC)
    assert [n for n, _ in calls] == ["qn_hmc_begin_s", "sse_grad", "noise_fold", "qn_hmc_leap_s", "qn_hmc_accept", "noise_gibbs",
                                     "qn_hmc_begin_s", "sse_grad", "noise_fold", "qn_hmc_leap_s", "qn_hmc_accept"]
