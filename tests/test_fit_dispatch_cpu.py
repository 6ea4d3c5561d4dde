"""CPU: the refusal rules of the device engines are stated once, in `check_params`, and `NN_MCMC.fit(engine='device')` asks them
there.  A table of (sampler, settings) pairs that each break ONE rule: the engine's `check_params` and `fit` raise the same
exception type with the same message, and neither touches a device (the library loader, the solver's operator and torch's CUDA
initialisation are trapped); each pair's valid counterpart passes `check_params`.  And the `shard_params` hook that cuts the
per-chain sampler parameters to a rank's chains."""
import numpy as np
import pytest
import torch

from quinn_amd import _lib
from quinn_amd.solvers.nn_mcmc import DEVICE_ENGINES, NN_MCMC

NMCMC, C = 10, 4
HP, NP = dict(a0=3, b0=3), dict(a0=3, b0=1)


def _case(sampler, bad, good, net='mlp', dtype='float64', good_net=None, good_dtype=None, good_sampler=None, **fit_kw):
    """One row: `bad` / `good` are the sampler_params, or a dict of fit keywords when they hold the key 'fit'."""
    split = lambda d: (d['fit'], d.get('sp', {})) if 'fit' in d else ({}, d)
    (bkw, bsp), (gkw, gsp) = split(bad), split(good)
    return ((sampler, net, dtype, dict(fit_kw, **bkw), bsp),
            (good_sampler or sampler, good_net or net, good_dtype or dtype, dict(fit_kw, **gkw), gsp))


CASES = {
    "hyperprior with a ladder": _case('hmc', {'ladder': 2}, {}, hyperprior=HP),
    "hyperprior with use_graph": _case('mala', {'use_graph': True}, {'use_graph': False}, hyperprior=HP),
    "hyperprior on an RNet": _case('hmc', {}, {}, net='rnet', good_net='mlp', hyperprior=HP),
    "hyperprior with amcmc": _case('amcmc', {}, {}, good_sampler='hmc', hyperprior=HP),
    "noiseprior with a ladder": _case('mala', {'ladder': 2}, {}, noiseprior=NP),
    "noiseprior with use_graph": _case('hmc', {'use_graph': True}, {'use_graph': False}, noiseprior=NP),
    "noiseprior on an RNet": _case('mala', {}, {}, net='rnet', good_net='mlp', noiseprior=NP),
    "noiseprior with amcmc": _case('amcmc', {}, {}, good_sampler='mala', noiseprior=NP),
    "noiseprior with float32": _case('hmc', {}, {}, dtype='float32', good_dtype='float64', noiseprior=NP),
    "ess without priorsigma": _case('ess', {'fit': {}}, {'fit': {'priorsigma': 1.0}}),
    "ess max_shrink=0": _case('ess', {'max_shrink': 0}, {'max_shrink': 4}, priorsigma=1.0),
    "nuts max_depth=0": _case('nuts', {'epsilon': 0.1, 'max_depth': 0}, {'epsilon': 0.1, 'max_depth': 5}),
    "nuts epsilon=-0.1": _case('nuts', {'epsilon': -0.1}, {'epsilon': 0.1}),
    "nuts adapt > nmcmc": _case('nuts', {'adapt': NMCMC + 1}, {'adapt': NMCMC}),
    "nuts ladder=4": _case('nuts', {'ladder': 4}, {'ladder': None}),
    "nuts use_graph": _case('nuts', {'use_graph': True}, {'use_graph': False}),
    "nuts float32": _case('nuts', {}, {}, dtype='float32', good_dtype='float64'),
    "ladder that does not divide the chains": _case('hmc', {'ladder': 3}, {'ladder': 2}),
    "ladder with use_graph": _case('mala', {'ladder': 2, 'use_graph': True}, {'ladder': 2}),
    "hmc L=0": _case('hmc', {'L': 0}, {'L': 1}),
    "hmc target_accept=1.5": _case('hmc', {'adapt': 5, 'target_accept': 1.5}, {'adapt': 5, 'target_accept': 0.7}),
    "sghmc alpha=0": _case('sghmc', {'eta': 1e-4, 'alpha': 0.0}, {'eta': 1e-4, 'alpha': 0.5}),
    "sgld eta=0": _case('sgld', {'eta': 0.0}, {'eta': 1e-4}),
    "amcmc float32": _case('amcmc', {}, {}, dtype='float32', good_dtype='float64'),
    "amcmc hist_scale0=0": _case('amcmc', {'hist_scale0': 0}, {'hist_scale0': 64.0}),
}
# the exception type each rule raises today (everything refuses with ValueError but the float32 AMCMC)
TYPES = {k: ValueError for k in CASES}
TYPES["amcmc float32"] = NotImplementedError


def _solver(net, dtype):
    torch.manual_seed(0)
    if net == 'rnet':
        from quinn_amd.nns.rnet import RNet
        return NN_MCMC(RNet(4, 2, indim=1, outdim=1, layer_pre=True, layer_post=True), verbose=False, dtype=dtype)
    from quinn_amd.nns.mlp import MLP
    return NN_MCMC(MLP(1, 1, (4,), activ="tanh"), verbose=False, dtype=dtype)


@pytest.fixture
def no_device(monkeypatch):
    """Anything that would touch a device fails the test."""
    def trap(what):
        def f(*a, **k):
            raise AssertionError(f"{what} was called")
        return f
    monkeypatch.setattr(_lib, "lib", trap("_lib.lib"))
    monkeypatch.setattr(NN_MCMC, "_operator", trap("NN_MCMC._operator"))
    monkeypatch.setattr(torch.cuda, "_lazy_init", trap("torch.cuda._lazy_init"))
    was = torch.cuda.is_initialized()          # (False, unless an earlier test of the same process has used a GPU)
    yield
    assert torch.cuda.is_initialized() == was


def _check(uq, sampler, kw, sp):
    return DEVICE_ENGINES[sampler].check_params(uq.arch, uq._dtype, NMCMC, kw.get('priorsigma'), nchains=C,
                                                hyperprior=kw.get('hyperprior'), noiseprior=kw.get('noiseprior'), **sp)


@pytest.mark.parametrize("name", sorted(CASES))
def test_check_params_and_fit_refuse_alike_and_touch_no_device(name, no_device):
    (sampler, net, dtype, kw, sp), good = CASES[name]
    uq = _solver(net, dtype)
    with pytest.raises(TYPES[name]) as direct:
        _check(uq, sampler, kw, sp)
    assert type(direct.value) is TYPES[name]
    x = np.linspace(-1, 1, 8)[:, None]
    with pytest.raises(TYPES[name]) as through_fit:
        uq.fit(x, np.sin(x), zflag=False, nmcmc=NMCMC, param_ini=np.zeros((C, uq.pdim)), seeds=list(range(C)), sampler=sampler,
               engine='device', sampler_params=sp, **kw)
    assert type(through_fit.value) is type(direct.value) and str(through_fit.value) == str(direct.value)
    # the valid counterpart passes, and hands back the settings the constructor keeps
    gsampler, gnet, gdtype, gkw, gsp = good
    cfg = _check(_solver(gnet, gdtype), gsampler, gkw, gsp)
    assert cfg['priorsigma'] == gkw.get('priorsigma')


def test_check_params_returns_the_normalised_settings(no_device):
    uq = _solver('mlp', 'float64')
    cfg = _check(uq, 'hmc', dict(hyperprior=dict(HP, groups='layer'), noiseprior=NP, priorsigma=2), {'adapt': 5})
    assert cfg['hyperprior'] == dict(a0=3.0, b0=3.0, groups='layer', every=1, tau0=None)
    assert cfg['noiseprior'] == dict(a0=3.0, b0=1.0, every=1, sigma_init=None)
    assert cfg['prior_groups'] == [('layer0', 0, 8), ('layer1', 8, 13)] and cfg['seg'].tolist() == [0, 8, 13]
    assert cfg['priorsigma'] == 2.0 and cfg['adapt'] == 5 and cfg['target_accept'] == 0.8 and cfg['ladder'] is None
    assert _check(uq, 'mala', {}, {'adapt': 5})['target_accept'] == 0.574
    cfg = _check(uq, 'hmc', {}, {'ladder': 2, 'beta_min': 0.25})
    assert cfg['ladder'].tolist() == [1.0, 0.25] and cfg['hyperprior'] is None and cfg['prior_groups'] is None
    assert _check(uq, 'nuts', {}, {'epsilon': [0.1, 0.2], 'adapt': 3})['nuts'][1:] == (10, 3, 0.8, 32)
    assert _check(uq, 'ess', dict(priorsigma=2), {'block': 8})['ess'] == (2.0, 32, 8)


def test_hyperprior_and_noiseprior_are_refused_on_the_host_engines_in_the_same_words():
    uq = _solver('mlp', 'float64')
    x = np.linspace(-1, 1, 8)[:, None]
    for key, val in (('hyperprior', HP), ('noiseprior', NP)):
        with pytest.raises(ValueError) as host:
            uq.fit(x, np.sin(x), zflag=False, nmcmc=NMCMC, param_ini=np.zeros(uq.pdim), sampler='hmc', sampler_params={},
                   **{key: val})
        with pytest.raises(ValueError) as dev:
            _check(uq, 'sghmc', {key: val}, {})
        assert str(host.value) == f"{key} runs with sampler='hmc' | 'mala' and engine='device' only (got sampler='hmc', engine='host')"
        assert str(dev.value) == str(host.value).replace("sampler='hmc', engine='host'", "sampler='sghmc', engine='device'")


def test_shard_params_cuts_the_per_chain_nuts_parameters_and_nothing_else():
    eps, scale = np.arange(1, 7) / 10.0, np.arange(18.0).reshape(6, 3) + 1.0
    sp = {'epsilon': eps, 'mass_scale': scale, 'max_depth': 5}
    out = DEVICE_ENGINES['nuts'].shard_params(sp, 2, 5)
    assert np.array_equal(out['epsilon'], eps[2:5]) and np.array_equal(out['mass_scale'], scale[2:5]) and out['max_depth'] == 5
    assert out['epsilon'].dtype == np.float64 and sp['epsilon'] is eps and sp['mass_scale'] is scale      # (the input is left alone)
    out = DEVICE_ENGINES['nuts'].shard_params({'epsilon': 0.1, 'mass_scale': None, 'adapt': 3}, 2, 5)
    assert out == {'epsilon': 0.1, 'mass_scale': None, 'adapt': 3}
    out = DEVICE_ENGINES['nuts'].shard_params({'epsilon': list(eps)}, 0, 0)                               # a rank without chains
    assert out['epsilon'].shape == (0,)
    for sampler in ('amcmc', 'hmc', 'mala', 'sgld', 'sghmc', 'ess'):                                      # default: the identity
        assert DEVICE_ENGINES[sampler].shard_params(sp, 2, 5) is sp
