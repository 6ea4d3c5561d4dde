"""GPU: what a device engine declares about its result (`DeviceEngine._extra_keys`) against what its runs return.  For every
engine and every setting that adds result keys: (a) `empty_results(nmcmc)`, the result of a rank that owns no chain, has the keys
(in the order `gather_results` walks them on every rank), the numpy dtypes and the trailing shapes of a real run's result, and
the same scalars; (b) a run in two groups returns what a run in one returns; (c) the keys beyond the six common ones are those of
the literal table below, written down from the empty dicts `NN_MCMC.fit` and `parallel.empty_results` built by hand before the
engines declared them.  (1, 4, 1) tanh, 8 rows, float64, 4 chains, 6 steps (30 with a 25-step warm-up: a mass window needs 20)."""
import numpy as np
import pytest
import torch

from quinn_amd.mcmc.device_amcmc import DeviceAMCMC
from quinn_amd.mcmc.device_ess import DeviceESS
from quinn_amd.mcmc.device_hmc import DeviceHMC
from quinn_amd.mcmc.device_mala import DeviceMALA
from quinn_amd.mcmc.device_nuts import DeviceNUTS
from quinn_amd.mcmc.device_sgmcmc import DeviceSGHMC, DeviceSGLD
from quinn_amd.ops import BatchedMLP, MLPArch
from quinn_amd.parallel import gather_results

pytestmark = pytest.mark.gpu
ARCH = MLPArch((1, 4, 1), "tanh")
P, C = 13, 4
F64, I32, I64 = np.dtype(np.float64), np.dtype(np.int32), np.dtype(np.int64)
COMMON = {'chain': ((None, P), F64), 'mapparams': ((P,), F64), 'maxpost': ((), F64), 'accrate': ((), F64),
          'logpost': ((None,), F64), 'alphas': ((None,), F64)}                 # (None: nmcmc + 1)
HYPER, NOISE = dict(a0=3, b0=3, groups='layer', every=2), dict(a0=3, b0=1, every=3)
NUTS_KEYS = {'depth': ((7,), I32), 'nleap': ((7,), I32), 'ndiv': ((), I64), 'ntreedepth': ((), I64), 'ngrad': ((), I64),
             'epsilon': ((), F64)}

# name: (engine, nmcmc, its arguments, the result's keys beyond the common ones: (trailing shape, dtype) or the scalar / None)
CASES = {
    "amcmc": (DeviceAMCMC, 6, {}, {}),
    "hmc": (DeviceHMC, 6, dict(epsilon=0.01, L=2), {}),
    "mala": (DeviceMALA, 6, dict(epsilon=0.01), {}),
    "sgld": (DeviceSGLD, 6, dict(eta=1e-4, batch=4), {}),
    "sghmc": (DeviceSGHMC, 6, dict(eta=1e-4, batch=4), {}),
    "ess": (DeviceESS, 6, dict(priorsigma=1), {'nev': ((7,), I32), 'ntrunc': ((), I64), 'nevals': ((), I64)}),
    "nuts": (DeviceNUTS, 6, dict(epsilon=0.02, max_depth=3), dict(NUTS_KEYS, nwarm=0)),
    "nuts adapt=4": (DeviceNUTS, 6, dict(epsilon=0.02, max_depth=3, adapt=4), dict(NUTS_KEYS, nwarm=4)),
    "hmc adapt=25": (DeviceHMC, 30, dict(epsilon=0.01, L=2, adapt=25), {'epsilon': ((), F64), 'mass_scale': ((P,), F64), 'nwarm': 25}),
    "hmc adapt=25 adapt_mass=False": (DeviceHMC, 30, dict(epsilon=0.01, L=2, adapt=25, adapt_mass=False),
                                      {'epsilon': ((), F64), 'mass_scale': None, 'nwarm': 25}),
    "hmc ladder=2": (DeviceHMC, 6, dict(epsilon=0.01, L=2, ladder=2),
                     {'beta': ((), F64), 'swap_rate': ((), F64), 'replica': ((7,), I32)}),
    "hmc hyperprior": (DeviceHMC, 6, dict(epsilon=0.01, L=2, hyperprior=HYPER), {'tau': ((4, 2), F64)}),
    "hmc noiseprior": (DeviceHMC, 6, dict(epsilon=0.01, L=2, noiseprior=NOISE), {'sigma': ((3,), F64)}),
    "hmc hyperprior + noiseprior": (DeviceHMC, 6, dict(epsilon=0.01, L=2, hyperprior=HYPER, noiseprior=NOISE),
                                    {'tau': ((4, 2), F64), 'sigma': ((3,), F64)}),
    "hmc hyperprior + noiseprior every=0": (DeviceHMC, 6, dict(epsilon=0.01, L=2, hyperprior=dict(HYPER, every=0, tau0=1.0),
                                                               noiseprior=dict(every=0)),
                                            {'tau': ((1, 2), F64), 'sigma': ((1,), F64)}),
}


@pytest.fixture(scope="module")
def problem():
    rs = np.random.RandomState(0)
    x = np.linspace(-1, 1, 8)[:, None]
    return BatchedMLP(ARCH, x, np.sin(2 * x) + 0.1 * rs.randn(8, 1)), 0.3 * rs.randn(C, P)


def _signature(res):
    """[(key, None | the scalar | (trailing shape, numpy dtype))] of a result as `fit` stores it, and the rows of its arrays."""
    res = gather_results(res, C, 'none')
    sig = [(k, v if v is None or np.isscalar(v) else (v.shape[1:], v.dtype)) for k, v in res.items()]
    return sig, {len(v) for v in res.values() if isinstance(v, np.ndarray)}


@pytest.mark.parametrize("name", sorted(CASES))
def test_empty_grouped_and_plain_results_have_the_declared_keys(name, problem):
    cls, nmcmc, kw, extra = CASES[name]
    assert ARCH.nparams == P
    op, ini = problem
    eng = cls(op, 0.3, seed=5, **kw)
    run, rows = _signature(eng.run(nmcmc, ini))
    torch.cuda.synchronize()
    assert rows == {C}
    # (a) the result of a rank without chains
    empty, rows = _signature(eng.empty_results(nmcmc))
    assert rows == {0}
    assert empty == run
    # (b) two groups of two chains (whole ladders of two rungs, where there is a ladder)
    grouped, rows = _signature(cls(op, 0.3, seed=5, groups=2, **kw).run(nmcmc, ini))
    torch.cuda.synchronize()
    assert rows == {C} and grouped == run
    # (c) the table
    common = [(k, (tuple(nmcmc + 1 if n is None else n for n in tail), dt)) for k, (tail, dt) in COMMON.items()]
    assert run == common + list(extra.items())
