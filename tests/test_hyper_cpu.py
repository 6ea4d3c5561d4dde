"""CPU: the hierarchical weight prior's numpy contract (`quinn_amd.mcmc.hyper`) -- the law of `gamma_draw`, the consistency of
the cache a Gibbs round refreshes, the weight groups, every refusal of `check_hyperprior` and `NN_MCMC.fit`, and the two entry
points in the header and the binding.  No device is needed."""
import os

import numpy as np
import pytest
import torch

from quinn_amd import _lib
from quinn_amd.mcmc import hyper as hy
from quinn_amd.mcmc.sgmcmc import ctr_of, philox4x32
from quinn_amd.ops import MLPArch


@pytest.mark.parametrize("shape", [0.6, 1.0, 7.5])
def test_gamma_draw_samples_the_gamma_law(shape):
    """200 000 draws (one per chain id) at rate 2.5: mean within 5 SE of a / r, SE = sqrt(a / r^2 / n); variance within 5 SE of
    a / r^2, SE^2 = (mu_4 - sigma^4) / n with mu_4 = (3 a^2 + 6 a) / r^4."""
    n, r = 200_000, 2.5
    x = hy.gamma_draw(12345, 3, np.arange(n), 2, shape, r)
    assert x.shape == (n,) and np.all(x > 0) and np.isfinite(x).all()
    mean, var = x.mean(), x.var(ddof=1)
    se_m = np.sqrt(shape / r ** 2 / n)
    se_v = np.sqrt(((3 * shape ** 2 + 6 * shape) / r ** 4 - shape ** 2 / r ** 4) / n)
    print(shape, "mean", mean, "z", (mean - shape / r) / se_m, "var", var, "z", (var - shape / r ** 2) / se_v)
    assert abs(mean - shape / r) <= 5 * se_m
    assert abs(var - shape / r ** 2) <= 5 * se_v


def test_gamma_draw_is_keyed_by_seed_step_chain_and_group_and_broadcasts():
    a = hy.gamma_draw(7, 4, np.arange(6)[:, None], np.arange(3)[None, :], 2.5, np.full((6, 3), 1.5))
    assert a.shape == (6, 3)
    for c in range(6):
        for g in range(3):
            assert hy.gamma_draw(7, 4, c, g, 2.5, 1.5) == a[c, g]            # a draw does not depend on its neighbours
    flat = a.ravel()
    assert len(set(flat)) == flat.size
    assert hy.gamma_draw(8, 4, 0, 0, 2.5, 1.5) != a[0, 0] and hy.gamma_draw(7, 5, 0, 0, 2.5, 1.5) != a[0, 0]
    # the first attempt by hand: block 0 -> the normal, block 1 -> the uniform of the test
    shape, rate, c, g = 2.5, 1.5, 3, 1
    b0 = philox4x32(7, 2 * 4 + 1, ctr_of(c, 11, np.uint64(g << 16)))
    b1 = philox4x32(7, 2 * 4 + 1, ctr_of(c, 11, np.uint64((g << 16) | 1)))
    x = np.sqrt(-2.0 * np.log(hy.u01(b0[0], b0[1]))) * np.cos(6.283185307179586 * hy.u01(b0[2], b0[3]))
    d = shape - 1.0 / 3.0
    v = (1.0 + x / np.sqrt(9.0 * d)) ** 3
    if v > 0 and np.log(hy.u01(b1[0], b1[1])) < 0.5 * x * x + d - d * v + d * np.log(v):
        np.testing.assert_allclose(a[c, g], d * v / rate, rtol=1e-15)
    else:
        assert a[c, g] != d * v / rate


def _state(C=4, seg=(0, 5, 6, 30, 37), sigma=0.3, a0=2.0, b0=1.5, seed=0):
    rs = np.random.RandomState(seed)
    seg = np.asarray(seg, dtype=np.int64)
    p, G = int(seg[-1]), len(seg) - 1
    cur = rs.randn(C, p)
    glik, sse = 3.0 * rs.randn(C, p), 10.0 + 40.0 * rs.rand(C)               # the bare gradient and SSE of the likelihood
    tau = 0.5 + rs.rand(C, G)
    lam, c0 = hy.fold_constants_g(sigma, tau, seg, a0, b0)
    g, s = hy.fold_g(cur, lam, c0, seg, grad=glik, sse=sse)
    return dict(cur=cur, glik=glik, sse=sse, tau=tau, lam=lam, c0=c0, seg=seg, gcur=g, cur_lp=-0.5 * s / sigma ** 2 - 7.0,
                sigma=sigma, a0=a0, b0=b0)


def test_gibbs_round_keeps_the_cached_state_consistent():
    """The refreshed grad_cur and cur_lp equal those recomputed from scratch at the new precisions (`fold_g` on the bare
    gradient and SSE; `log_joint`), to 1e-12 of the largest entry."""
    st = _state()
    sigma, a0, b0, seg = st['sigma'], st['a0'], st['b0'], st['seg']
    r = hy.gibbs_round(st['cur'], st['gcur'], st['cur_lp'], st['lam'], st['c0'], seg, sigma, a0, b0, seed=11, step=6, chain0=5)
    assert r['ok'].all() and np.all(r['tau'] > 0) and not np.allclose(r['tau'], st['tau'])
    np.testing.assert_array_equal(r['lam'], sigma ** 2 * r['tau'])
    lam2, c02 = hy.fold_constants_g(sigma, r['tau'], seg, a0, b0)
    np.testing.assert_array_equal(lam2, r['lam'])
    np.testing.assert_allclose(c02, r['c0'], rtol=1e-15)
    g2, s2 = hy.fold_g(st['cur'], lam2, c02, seg, grad=st['glik'], sse=st['sse'])
    assert np.abs(r['grad_cur'] - g2).max() <= 1e-12 * np.abs(g2).max()
    want_lp = -0.5 * s2 / sigma ** 2 - 7.0
    assert np.abs(r['cur_lp'] - want_lp).max() <= 1e-12 * np.abs(want_lp).max()
    # ... and cur_lp is the joint density: (likelihood part) + log N(w; 0, 1 / tau) + log p(tau)
    joint = hy.log_joint(st['cur'], r['tau'], seg, a0, b0, loglik=-0.5 * st['sse'] / sigma ** 2 - 7.0)
    assert np.abs(r['cur_lp'] - joint).max() <= 1e-12 * np.abs(joint).max()
    # the draw is the conditional's: Gamma(a0 + n_g / 2, rate b0 + S_g / 2) with the documented key
    S = hy.group_sumsq(st['cur'], seg)
    n = np.diff(seg)
    for c in range(4):
        for g in range(4):
            assert r['tau'][c, g] == hy.gamma_draw(11, 6, 5 + c, g, a0 + n[g] / 2, b0 + S[c, g] / 2)


def test_gibbs_round_leaves_a_chain_with_a_non_finite_state_alone():
    st = _state()
    cur = st['cur'].copy()
    cur[1, 17] = np.nan
    clean = hy.gibbs_round(st['cur'], st['gcur'], st['cur_lp'], st['lam'], st['c0'], st['seg'], 0.3, 2.0, 1.5, 11, 6, 5)
    r = hy.gibbs_round(cur, st['gcur'], st['cur_lp'], st['lam'], st['c0'], st['seg'], 0.3, 2.0, 1.5, 11, 6, 5)
    assert list(r['ok']) == [True, False, True, True]
    for k, old in (('lam', st['lam']), ('c0', st['c0']), ('cur_lp', st['cur_lp']), ('grad_cur', st['gcur'])):
        np.testing.assert_array_equal(r[k][1], old[1])
        np.testing.assert_array_equal(r[k][[0, 2, 3]], clean[k][[0, 2, 3]])
    np.testing.assert_allclose(r['tau'][1], st['tau'][1], rtol=1e-15)


def test_the_conditional_of_tau_has_the_conjugate_moments():
    """Many chains at ONE state: the draws' mean is (a0 + n / 2) / (b0 + S / 2) within 5 SE."""
    C, seg = 20000, np.array([0, 3, 10])
    w = np.tile(np.random.RandomState(1).randn(10), (C, 1))
    lam, c0 = hy.fold_constants_g(1.0, np.ones((C, 2)), seg, 2.0, 1.0)
    r = hy.gibbs_round(w, np.zeros_like(w), np.zeros(C), lam, c0, seg, 1.0, 2.0, 1.0, seed=3, step=0)
    S = hy.group_sumsq(w[:1], seg)[0]
    shape, rate = 2.0 + np.array([3, 7]) / 2, 1.0 + S / 2
    assert np.all(np.abs(r['tau'].mean(axis=0) - shape / rate) <= 5 * np.sqrt(shape / rate ** 2 / C))


def test_group_segments():
    from quinn_amd.nns.mlp import MLP
    arch = MLPArch.from_module(MLP(2, 1, (5, 3)))
    assert arch.dims == (2, 5, 3, 1) and arch.nparams == 37
    seg, names = hy.group_segments(arch, 'layer')
    assert seg.dtype == np.int64 and seg.tolist() == [0, 15, 33, 37] and names == ['layer0', 'layer1', 'layer2']
    seg, names = hy.group_segments(arch, 'tensor')
    assert seg.tolist() == [0, 10, 15, 30, 33, 36, 37] and names == ['W0', 'b0', 'W1', 'b1', 'W2', 'b2']
    seg, names = hy.group_segments(arch, 'all')
    assert seg.tolist() == [0, 37] and names == ['all']
    seg, names = hy.group_segments(MLPArch((2, 5, 1), bias=False), 'tensor')
    assert seg.tolist() == [0, 10, 15] and names == ['W0', 'W1']
    with pytest.raises(ValueError, match="'layer', 'tensor' or 'all'"):
        hy.group_segments(arch, 'ard')
    deep = MLPArch((1,) + (2,) * 32 + (1,))                                   # 33 layers, 66 tensors
    with pytest.raises(ValueError, match="at most 32"):
        hy.group_segments(deep, 'layer')
    with pytest.raises(ValueError, match="at most 32"):
        hy.group_segments(deep, 'tensor')
    assert len(hy.group_segments(MLPArch((1,) + (2,) * 31 + (1,)), 'layer')[1]) == 32
    assert hy.group_segments(deep, 'all')[0].tolist() == [0, deep.nparams]
    for bad in ([0, 5], [1, 37], [0, 5, 5, 37], [0, 9, 5, 37], np.arange(35)):
        with pytest.raises(ValueError):
            hy.check_segments(bad, 37)
    assert hy.check_segments([0, 5, 37], 37).dtype == np.int64


def test_check_hyperprior_and_initial_tau():
    assert hy.check_hyperprior(None) is None
    hp = hy.check_hyperprior(dict(a0=3, b0=2))
    assert hp == {'a0': 3.0, 'b0': 2.0, 'groups': 'layer', 'every': 1, 'tau0': None}
    assert hy.check_hyperprior(hp) == hp                                      # (its own output is accepted: engines clone)
    assert hy.initial_tau(hp, 3).tolist() == [1.5] * 3                        # a0 / b0
    assert hy.initial_tau(hp, 3, priorsigma=0.5).tolist() == [4.0] * 3        # 1 / priorsigma^2
    assert hy.initial_tau(hy.check_hyperprior(dict(a0=3, b0=2, tau0=7)), 2, priorsigma=0.5).tolist() == [7.0, 7.0]
    assert hy.initial_tau(hy.check_hyperprior(dict(a0=3, b0=2, tau0=[1, 2], every=0)), 2).tolist() == [1.0, 2.0]
    with pytest.raises(ValueError, match="2 values for 3 groups"):
        hy.initial_tau(hy.check_hyperprior(dict(a0=3, b0=2, tau0=[1, 2])), 3)
    for bad, msg in [("layer", "None or a dict"), (dict(b0=1), "needs a0"), (dict(a0=1), "needs b0"),
                     (dict(a0=0, b0=1), "a0"), (dict(a0=1, b0=-2), "b0"), (dict(a0=np.inf, b0=1), "a0"),
                     (dict(a0=np.nan, b0=1), "a0"), (dict(a0="1", b0=1), "a0"), (dict(a0=True, b0=1), "a0"),
                     (dict(a0=[1, 2], b0=1), "a0"), (dict(a0=1, b0=1, groups='ard'), "groups"),
                     (dict(a0=1, b0=1, groups=3), "groups"), (dict(a0=1, b0=1, every=-1), "every"),
                     (dict(a0=1, b0=1, every=1.5), "every"), (dict(a0=1, b0=1, every=True), "every"),
                     (dict(a0=1, b0=1, every=0), "needs tau0"), (dict(a0=1, b0=1, tau0=0), "tau0"),
                     (dict(a0=1, b0=1, tau0=[1, -1]), "tau0"), (dict(a0=1, b0=1, tau0=[]), "tau0"),
                     (dict(a0=1, b0=1, tau0=np.nan), "tau0"), (dict(a0=1, b0=1, ard=True), "unknown keys")]:
        with pytest.raises(ValueError, match=msg):
            hy.check_hyperprior(bad)


def _solver(rnet=False):
    from quinn_amd.solvers.nn_mcmc import NN_MCMC
    torch.manual_seed(0)
    if rnet:
        from quinn_amd.nns.rnet import RNet
        return NN_MCMC(RNet(4, 2, indim=1, outdim=1, layer_pre=True, layer_post=True), verbose=False)
    from quinn_amd.nns.mlp import MLP
    return NN_MCMC(MLP(1, 1, (4,), activ="tanh"), verbose=False)


FIT_REFUSALS = [
    (dict(sampler='amcmc', engine='device'), "sampler='hmc' | 'mala' and engine='device' only"),
    (dict(sampler='nuts', engine='device'), "sampler='hmc' | 'mala' and engine='device' only"),
    (dict(sampler='ess', engine='device', priorsigma=1.0), "sampler='hmc' | 'mala' and engine='device' only"),
    (dict(sampler='sgld', engine='device'), "sampler='hmc' | 'mala' and engine='device' only"),
    (dict(sampler='hmc', engine='host'), "sampler='hmc' | 'mala' and engine='device' only"),
    (dict(sampler='mala', engine='host'), "sampler='hmc' | 'mala' and engine='device' only"),
    (dict(sampler='hmc', engine='device', sampler_params={'ladder': 2}), "ladder"),
    (dict(sampler='mala', engine='device', sampler_params={'use_graph': True}), "use_graph"),
    (dict(sampler='hmc', engine='device', hyperprior=dict(a0=1, b0=1, tau0=[1, 2, 3])), "3 values for 2 groups"),
    (dict(sampler='hmc', engine='device', hyperprior=dict(a0=1, b0=1, every=0)), "needs tau0"),
    (dict(sampler='hmc', engine='device', hyperprior=dict(a0=-1, b0=1)), "a0"),
    (dict(sampler='hmc', engine='device', hyperprior=3.0), "None or a dict"),
]


@pytest.mark.parametrize("kw,msg", FIT_REFUSALS)
def test_fit_refuses_before_any_device_is_touched(kw, msg):
    uq = _solver()
    x = np.linspace(-1, 1, 8)[:, None]
    kw = dict(dict(hyperprior=dict(a0=3, b0=3), sampler_params={}), **kw)
    with pytest.raises(ValueError, match=msg):
        uq.fit(x, np.sin(x), zflag=False, nmcmc=10, param_ini=np.zeros((2, uq.pdim)), seeds=[0, 1], **kw)


def test_fit_refuses_a_residual_network():
    uq = _solver(rnet=True)
    x = np.linspace(-1, 1, 8)[:, None]
    with pytest.raises(ValueError, match="residual network"):
        uq.fit(x, np.sin(x), zflag=False, nmcmc=10, param_ini=np.zeros((2, uq.pdim)), seeds=[0, 1], sampler='hmc',
               engine='device', sampler_params={}, hyperprior=dict(a0=3, b0=3))


def test_hyperprior_is_keyword_only_in_fit():
    import inspect
    from quinn_amd.solvers.nn_mcmc import NN_MCMC
    par = inspect.signature(NN_MCMC.fit).parameters['hyperprior']
    assert par.kind is inspect.Parameter.KEYWORD_ONLY and par.default is None


def test_the_header_lists_both_entry_points_and_the_binding_has_them():
    import ctypes
    fold, gibbs = _lib.FUNCTIONS['qn_prior_fold_g'], _lib.FUNCTIONS['qn_hyper_gibbs']
    v, i, i64, u64, d = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_uint64, ctypes.c_double
    assert fold == (i, [v, v, v, v, i, v, i, v, i, i, i64, v])
    assert gibbs == (i, [v] * 10 + [d, d, d, i, i, i, i, i, i64, i, u64, i, i, v])
    assert 'qn_hyper.hip' in _lib.SOURCES
    assert os.path.exists(os.path.join(_lib.CSRC, 'qn_hyper.hip'))
    if os.path.exists(_lib.LIBPATH):                                           # (built: the library exports and binds them)
        L = _lib.lib()
        assert L.qn_prior_fold_g.argtypes == fold[1] and L.qn_hyper_gibbs.argtypes == gibbs[1]
