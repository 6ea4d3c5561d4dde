"""CPU: the Gaussian weight prior's contract (`quinn_amd.mcmc.prior`) that qn_prior_fold and the engines are checked against --
the fold identities against a direct evaluation of loglik + log N(w; 0, ps^2 I), the minibatch constants, the refusals of
`check_priorsigma`, of qn_prior_fold (they need no device) and of `NN_MCMC.fit`."""
import numpy as np
import pytest
from scipy.stats import norm

from quinn_amd import _lib
from quinn_amd.mcmc import prior as pr


def test_fold_is_the_log_posterior_with_the_prior_and_its_gradient():
    """sse' and g' of `fold`, pushed through the samplers' gs = -0.5 / sigma^2 and constant, against loglik + log prior written
    out with scipy on a linear model y = A w + noise (where SSE and its gradient are closed forms)."""
    rs = np.random.RandomState(0)
    N, p, C = 11, 7, 5
    A, y = rs.randn(N, p), rs.randn(N)
    for sigma, ps in ((0.3, 0.8), (1.7, 0.05), (0.02, 12.0)):
        W = ps * rs.randn(C, p)
        res = W @ A.T - y                                         # [C, N]
        sse, g = np.sum(res ** 2, axis=1), 2.0 * res @ A          # SSE and d SSE / d W
        lam, c0 = pr.fold_constants(sigma, ps, p)
        g2, sse2 = pr.fold(W, lam, c0, grad=g, sse=sse)
        gs = -0.5 / sigma ** 2
        got_lp = gs * sse2 - (N / 2) * np.log(2 * np.pi) - N * np.log(sigma)
        want_lp = norm.logpdf(y[None, :], loc=W @ A.T, scale=sigma).sum(axis=1) + norm.logpdf(W, loc=0.0, scale=ps).sum(axis=1)
        np.testing.assert_allclose(got_lp, want_lp, rtol=1e-12)
        want_g = -(res @ A) / sigma ** 2 - W / ps ** 2
        np.testing.assert_allclose(gs * g2, want_g, rtol=1e-12, atol=1e-12 * np.abs(want_g).max())
        np.testing.assert_allclose(pr.log_prior(W, ps), norm.logpdf(W, loc=0.0, scale=ps).sum(axis=1), rtol=1e-12)
        np.testing.assert_allclose(pr.grad_log_prior(W, ps), -W / ps ** 2, rtol=1e-15)
        # None stays None; a float32 gradient is widened, updated in float64 and rounded once
        assert pr.fold(W, lam, c0) == (None, None)
        g32 = g.astype(np.float32)
        out32, _ = pr.fold(W, lam, c0, grad=g32)
        assert out32.dtype == np.float32 and np.array_equal(out32, (g32.astype(np.float64) + (2 * lam) * W).astype(np.float32))
        assert np.array_equal(pr.fold(W, lam, c0, grad=g)[0], g + (2 * lam) * W)


def test_fold_constants_with_a_minibatch_leave_the_prior_unscaled():
    rs = np.random.RandomState(1)
    w = rs.randn(3, 9)
    sigma, ps, p = 0.4, 0.7, 9
    lam, c0 = pr.fold_constants(sigma, ps, p)
    assert lam == sigma ** 2 / ps ** 2 and np.isclose(c0, sigma ** 2 * p * np.log(2 * np.pi * ps ** 2), rtol=1e-15)
    full = lam * np.sum(w * w, axis=1) + c0
    for n_rows, n_batch in ((64, 16), (1000, 7), (48, 48)):
        lb, cb = pr.fold_constants(sigma, ps, p, n_rows=n_rows, n_batch=n_batch)
        np.testing.assert_allclose((n_rows / n_batch) * (lb * np.sum(w * w, axis=1) + cb), full, rtol=1e-14)
    assert pr.fold_constants(sigma, ps, p, n_rows=48, n_batch=48) == (lam, c0)
    with pytest.raises(ValueError):
        pr.fold_constants(sigma, None, p)


def test_check_priorsigma():
    assert pr.check_priorsigma(None) is None
    assert pr.check_priorsigma(2) == 2.0 and isinstance(pr.check_priorsigma(2), float)
    assert pr.check_priorsigma(np.float64(0.5)) == 0.5
    for bad in (0, 0.0, -1, -0.3, float('nan'), float('inf'), -float('inf'), "1.0", "wide", True, [1.0], (0.5, 0.5)):
        with pytest.raises(ValueError):
            pr.check_priorsigma(bad)


def test_c_abi_symbol_and_refusals_without_a_device():
    _lib.build()
    L = _lib.lib()
    assert "qn_prior_fold" in _lib.SYMBOLS and hasattr(L, "qn_prior_fold")
    one = 8                                                                # a non-NULL pointer that is never touched
    ok = dict(W=one, lam=0.37, c0=-1.25, grad=one, gdtype=_lib.QN_F64, sse=one, sse_stride=1, C=3, p=7, stream=None)
    nan, inf = float('nan'), float('inf')
    for bad in (dict(W=None), dict(grad=None, sse=None), dict(lam=0.0), dict(lam=-1.0), dict(lam=nan), dict(lam=inf),
                dict(c0=nan), dict(c0=inf), dict(c0=-inf), dict(C=0), dict(C=-1), dict(C=65536), dict(p=0), dict(p=-5),
                dict(sse_stride=0), dict(sse_stride=-2), dict(gdtype=2), dict(gdtype=-1)):
        args = dict(ok, **bad)
        assert L.qn_prior_fold(*args.values()) == -1, bad
        assert b"qn_prior_fold" in L.qn_last_error(), bad


def test_fit_refuses_a_bad_priorsigma_before_any_launch():
    from quinn_amd.nns.mlp import MLP
    from quinn_amd.solvers.nn_mcmc import NN_MCMC
    s = NN_MCMC(MLP(1, 1, (4,), activ="tanh"), verbose=False)
    x, y = np.linspace(-1, 1, 8)[:, None], np.zeros((8, 1))
    for bad in (-1, 0, float('nan'), "0.5"):
        for engine in ("host", "device"):
            with pytest.raises(ValueError, match="priorsigma"):
                s.fit(x, y, zflag=False, nmcmc=5, param_ini=np.zeros(s.pdim), sampler='hmc', sampler_params={'epsilon': 0.01},
                      engine=engine, priorsigma=bad)
    assert s._op is None                                                   # no operator was built: nothing was launched
