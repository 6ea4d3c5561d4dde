"""CPU: the contract of elliptical slice sampling (`quinn_amd.mcmc.ess`) -- the numpy restatement samples a Gaussian posterior
exactly, truncation keeps the target, a non-finite SSE is never accepted, and bad arguments are refused before any device is
touched."""
import numpy as np
import pytest

from quinn_amd.mcmc import ess

SIGMA, S, N = 0.5, 1.0, 32
# 3 x the largest deviation of five other seeds (below): pooled mean / covariance in units of the marginal standard deviations
BAR_MEAN, BAR_COV = 3 * 0.0309, 3 * 0.0285


def linear_problem():
    """y = x . (0.7, -0.4) + 0.3 + noise on 32 rows: the 3-dimensional Gaussian likelihood of the tests (2 weights and a bias)."""
    rs = np.random.RandomState(0)
    x = rs.rand(N, 2) * 2 - 1
    y = x @ np.array([0.7, -0.4]) + 0.3 + SIGMA * rs.randn(N)
    return x, y


def run_restatement(seed, C, nmcmc, max_shrink):
    """C chains of the numpy restatement from w = 0 with host-drawn partners and uniforms, the first tenth of every chain
    dropped: (dm, dc) of `ess.moment_deviation` against the closed form, and the number of truncated steps."""
    x, y = linear_problem()
    X = np.hstack([x, np.ones((N, 1))])
    mean, cov = ess.gaussian_posterior(X, y, SIGMA, S)
    sse = lambda w: float(np.sum((y - X @ w) ** 2))
    out, ntrunc = [], 0
    for c in range(C):
        r = ess.ess_chain(sse, np.zeros(3), SIGMA, S, N, nmcmc, max_shrink, np.random.RandomState(1000 * seed + c))
        assert r['nev'][1:].sum() == r['nevals'] and r['nev'][1:].min() >= 1 and r['nev'][1:].max() <= max_shrink
        out.append(r['chain'][nmcmc // 10:])
        ntrunc += r['ntrunc']
    return ess.moment_deviation(np.concatenate(out), mean, cov), ntrunc


def test_restatement_samples_the_gaussian_posterior():
    """8 chains x 4000 steps, seed 0.  Measured with the five other seeds 1 .. 5 (this function, same counts): dm = 0.0233,
    0.0309, 0.0222, 0.0084, 0.0165 and dc = 0.0221, 0.0187, 0.0129, 0.0091, 0.0285; no truncated step.  The bars are 3 x the
    largest of each: 0.0927 and 0.0855."""
    (dm, dc), ntrunc = run_restatement(0, 8, 4000, 32)
    print("dm = %.4f dc = %.4f ntrunc = %d" % (dm, dc, ntrunc))
    assert ntrunc == 0
    assert dm <= BAR_MEAN and dc <= BAR_COV


def test_truncation_keeps_the_target():
    """max_shrink = 1: a step is one proposal, 94 % of the steps are truncated and the chain stays -- and the mean is still
    within the bar of the untruncated test (the argument in `quinn_amd.mcmc.ess`).  A chain that moves in 6 % of its steps
    needs more of them for the same information: 8 chains x 16000 steps, one evaluation each.  Measured with seeds 1 .. 5: dm =
    0.0136, 0.0528, 0.0404, 0.0247, 0.0455."""
    (dm, _), ntrunc = run_restatement(0, 8, 16000, 1)
    print("dm = %.4f ntrunc = %d of %d" % (dm, ntrunc, 8 * 16000))
    assert 0.9 * 8 * 16000 < ntrunc < 8 * 16000
    assert dm <= BAR_MEAN


def _state(p=3):
    cur, nu = np.arange(1.0, p + 1), np.ones(p)
    st = {'cur': cur, 'nu': nu, 'sse_cur': 2.0, 'lp_cur': -5.0, 't': 0, 'ntrunc': 0, 'nevals': 0, 'best': cur.copy(), 'best_lp': -5.0}
    st.update(ess.ess_begin(cur, 2.0, nu, 0.3, 0.5, SIGMA))
    return st


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_a_non_finite_sse_is_never_accepted(bad):
    st = _state()
    st['logy'] = -np.inf                                          # even the lowest slice level does not let it in
    new, event = ess.ess_iter(st, bad, SIGMA, S, N, 10, 32, u_shrink=0.25)
    assert event == 'shrink' and new['j'] == 1 and new['t'] == 0 and new['nevals'] == 1
    assert np.array_equal(new['cur'], st['cur']) and new['sse_cur'] == 2.0 and new['lp_cur'] == -5.0
    assert new['tmax'] == st['theta'] and new['tmin'] == st['tmin']             # theta >= 0 at j = 0: the bracket shrinks from the right
    assert new['theta'] == new['tmin'] + 0.25 * (new['tmax'] - new['tmin'])
    # at the last proposal of the step it is a truncation: the chain stays and the step is counted
    st['j'] = 31
    new, event = ess.ess_iter(st, bad, SIGMA, S, N, 10, 32, nu_next=np.ones(3), u_next=(0.1, 0.9))
    assert event == 'trunc' and new['t'] == 1 and new['ntrunc'] == 1 and new['j'] == 0
    assert new['row'][0] == 1 and np.array_equal(new['row'][1], st['cur']) and new['row'][2] == -5.0 and new['row'][3] == 32


def test_an_iteration_accepts_shrinks_and_finishes():
    st = _state()
    gs = -0.5 / SIGMA ** 2
    assert st['logy'] == gs * 2.0 + np.log(0.5) and st['tmin'] == st['theta'] - 2 * np.pi and st['tmax'] == st['theta']
    acc, event = ess.ess_iter(st, 1.0, SIGMA, S, N, 2, 32, nu_next=np.full(3, 2.0), u_next=(0.6, 0.7))
    assert event == 'accept' and acc['t'] == 1 and np.array_equal(acc['cur'], st['prop']) and acc['sse_cur'] == 1.0
    assert acc['lp_cur'] == ess.log_post(1.0, np.sum(st['prop'] ** 2), 3, N, SIGMA, S) and acc['row'][3] == 1
    assert acc['theta'] == 2 * np.pi * 0.6 and acc['logy'] == gs * 1.0 + np.log(0.7) and acc['j'] == 0
    assert np.array_equal(acc['prop'], ess.ellipse(acc['cur'], np.full(3, 2.0), acc['theta']))
    last, event = ess.ess_iter(acc, 0.5, SIGMA, S, N, 2, 32)           # the last step: no next step is started, nothing is drawn
    assert event == 'accept' and last['t'] == 2 and np.array_equal(last['prop'], acc['prop'])
    done, event = ess.ess_iter(last, 0.0, SIGMA, S, N, 2, 32)
    assert event == 'done' and done['nevals'] == 2 and done['t'] == 2
    # a shrink from the left: theta < 0 moves tmin
    st['theta'] = -1.0
    left, event = ess.ess_iter(st, 1e9, SIGMA, S, N, 2, 32, u_shrink=0.5)
    assert event == 'shrink' and left['tmin'] == -1.0 and left['tmax'] == st['tmax']


def test_uniforms_are_philox_words():
    from quinn_amd.mcmc.sgmcmc import ctr_of, philox4x32
    w = philox4x32(5, 3, ctr_of(np.uint64(9), 8, np.uint64(0)))
    ut, uy = ess.start_uniforms(5, 3, 9)
    assert ut == ess.u01(w[0], w[1]) and uy == ess.u01(w[2], w[3]) and 0.0 < ut < 1.0
    w = philox4x32(5, 3, ctr_of(np.uint64(9), 8, np.uint64(4)))
    assert ess.shrink_uniform(5, 3, 9, 4) == ess.u01(w[0], w[1])
    assert ess.shrink_uniform(5, 3, 9, 4) != ess.shrink_uniform(5, 3, 9, 5) != ess.shrink_uniform(5, 4, 9, 4)


def test_gaussian_posterior_is_the_normal_equations():
    x, y = linear_problem()
    X = np.hstack([x, np.ones((N, 1))])
    mean, cov = ess.gaussian_posterior(X, y, SIGMA, S)
    g = X.T @ (y - X @ mean) / SIGMA ** 2 - mean / S ** 2             # the gradient of the log-posterior vanishes at the mean
    assert np.max(np.abs(g)) < 1e-10
    assert np.allclose(cov @ (X.T @ X / SIGMA ** 2 + np.eye(3) / S ** 2), np.eye(3), atol=1e-12)


@pytest.mark.parametrize("args", [(None, 32, 32), (0.0, 32, 32), (-1.0, 32, 32), (np.inf, 32, 32), (np.nan, 32, 32), ("1", 32, 32),
                                  (1.0, 0, 32), (1.0, 1.5, 32), (1.0, True, 32), (1.0, 32, 0), (1.0, 32, 2.0), (1.0, 32, None)])
def test_check_ess_args_refuses(args):
    with pytest.raises(ValueError):
        ess.check_ess_args(*args)


def test_check_ess_args_accepts():
    assert ess.check_ess_args(2, 1, 1) == (2.0, 1, 1)
    assert ess.check_ess_args(0.5, np.int64(32), 64) == (0.5, 32, 64)


def test_fit_refuses_before_any_device_is_touched(monkeypatch):
    """sampler='ess' without priorsigma, with engine='host', or with bad sampler_params: ValueError, and no operator is built."""
    from quinn_amd.nns.mlp import MLP
    from quinn_amd.solvers.nn_mcmc import NN_MCMC
    uq = NN_MCMC(MLP(1, 1, (4,), activ="tanh"), verbose=False)

    def touched(*a, **k):
        raise AssertionError("the device operator was built")
    monkeypatch.setattr(uq, "_operator", touched)
    x, y = np.zeros((4, 1)), np.zeros((4, 1))
    kw = dict(zflag=False, nmcmc=5, param_ini=np.zeros(uq.pdim))
    with pytest.raises(ValueError, match="priorsigma"):
        uq.fit(x, y, sampler='ess', engine='device', sampler_params={}, **kw)
    with pytest.raises(ValueError, match="engine='device'"):
        uq.fit(x, y, sampler='ess', engine='host', priorsigma=1.0, sampler_params={}, **kw)
    with pytest.raises(ValueError, match="max_shrink"):
        uq.fit(x, y, sampler='ess', engine='device', priorsigma=1.0, sampler_params={'max_shrink': 0}, **kw)


def ess_abi_cases():
    """(entry point, good arguments, bad changes) of the two entry points; pointers are the never-touched address 8."""
    from quinn_amd import _lib
    one, nan, inf = 8, float('nan'), float('inf')
    begin = dict(cur=one, sse_cur=one, lp_cur=one, sigma=0.5, priorsigma=1.0, C=3, chain0=0, p=7, seed=1, nu=one, prop=one,
                 prop_op=None, dtype=_lib.QN_F64, sq_parts=one, es=one, ei=one, stream=None)
    it = dict(sse_prop=one, nparts=1, sigma=0.5, priorsigma=1.0, n_rows=4, max_shrink=32, C=3, chain0=0, p=7, nmcmc=5, seed=1,
              cur=one, nu=one, prop=one, prop_op=None, dtype=_lib.QN_F64, best=one, best_lp=one, chain=None, lps=one, nev=one,
              sq_parts=one, es=one, ei=one, parity=0, stream=None)
    common = [dict(C=0), dict(C=65536), dict(C=-1), dict(p=0), dict(p=-3), dict(chain0=-1), dict(sigma=0.0), dict(sigma=nan),
              dict(sigma=inf), dict(priorsigma=0.0), dict(priorsigma=-1.0), dict(priorsigma=nan), dict(priorsigma=inf),
              dict(dtype=2), dict(prop_op=one), dict(cur=None), dict(nu=None), dict(prop=None), dict(sq_parts=None),
              dict(es=None), dict(ei=None)]
    return [("qn_ess_begin", begin, common + [dict(sse_cur=None), dict(lp_cur=None)]),
            ("qn_ess_iter", it, common + [dict(nmcmc=0), dict(max_shrink=0), dict(nparts=0), dict(n_rows=0), dict(parity=2),
                                          dict(parity=-1), dict(sse_prop=None), dict(best=None), dict(best_lp=None),
                                          dict(lps=None), dict(nev=None)])]


def test_c_abi_symbols_and_refusals_without_a_device():
    from quinn_amd import _lib
    _lib.build()
    L = _lib.lib()
    for name, ok, bads in ess_abi_cases():
        assert name in _lib.SYMBOLS and hasattr(L, name)
        for bad in bads:
            assert getattr(L, name)(*dict(ok, **bad).values()) == _lib.CONSTANTS["QN_EINVAL"], (name, bad)
            assert name.encode() in L.qn_last_error(), (name, bad)
