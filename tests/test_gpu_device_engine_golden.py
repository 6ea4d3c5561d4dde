"""GPU: the device samplers (DeviceAMCMC, DeviceHMC, DeviceMALA) reproduce, bit for bit, the chains recorded in
tests/golden/g17_device_engines.npz before the engines were put on one base class (quinn_amd/mcmc/device_engine.py).  The
engines use no atomics and sum in a fixed order, so a recording is reproducible; golden/gen_golden_device_engines.py writes
the file from `CASES` / `run_case` below."""
import os

import numpy as np
import pytest
import torch

from quinn_amd.mcmc.device_amcmc import DeviceAMCMC
from quinn_amd.mcmc.device_hmc import DeviceHMC
from quinn_amd.mcmc.device_mala import DeviceMALA
from quinn_amd.ops import BatchedMLP, MLPArch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g17_device_engines.npz")
DIMS, N, C, CHAIN0, SIGMA, SEED = (1, 8, 8, 1), 32, 4, 3, 0.2, 4321
KEYS = ('logpost', 'alphas', 'accrate', 'maxpost', 'mapparams')
# name: (engine, constructor arguments, nmcmc).  amcmc: one initial window, one adapted window of 64 + 16 steps (the look-ahead
# block path), an adapted tail, no compression; hmc, mala: a step size at which the chains both accept and reject; hmc_adapt: warmup_plan(30) closes its mass window at step 27
_AMCMC = dict(t0=10, tadapt=80)
_ADAPT = dict(epsilon=0.003, L=2, adapt=30)
CASES = {'amcmc_g1': (DeviceAMCMC, dict(_AMCMC, groups=1), 200),
         'amcmc_g2': (DeviceAMCMC, dict(_AMCMC, groups=2), 200),
         'hmc': (DeviceHMC, dict(epsilon=0.03, L=3), 40),
         'mala': (DeviceMALA, dict(epsilon=0.03), 40),
         'hmc_adapt': (DeviceHMC, _ADAPT, 40),
         'hmc_adapt_graph': (DeviceHMC, dict(_ADAPT, use_graph=True), 40)}


def run_case(name):
    """The arrays the fixture holds for case `name` ({key: numpy array})."""
    cls, kw, nmcmc = CASES[name]
    rs = np.random.RandomState(17)
    x = rs.rand(N, 1) * 6 - 3
    y = np.sin(x) + 0.1 * rs.randn(N, 1)
    arch = MLPArch(DIMS, "tanh")
    ini = 0.3 * rs.randn(C, arch.nparams)
    r = cls(BatchedMLP(arch, x, y), SIGMA, seed=SEED, chain0=CHAIN0, **kw).run(nmcmc, ini)
    torch.cuda.synchronize()
    out = {k: r[k].cpu().numpy() for k in KEYS}
    out['chain'] = r['chain'][:, ::20].cpu().numpy()
    if kw.get('adapt'):
        out.update(epsilon=r['epsilon'].cpu().numpy(), mass_scale=r['mass_scale'].cpu().numpy())
    return out


@pytest.fixture(scope="module")
def recorded(golden):
    return golden(os.path.basename(GOLDEN))


@pytest.mark.parametrize("name", list(CASES))
def test_engine_reproduces_the_recorded_chains(recorded, name):
    got = run_case(name)
    want = {k[len(name) + 1:]: v for k, v in recorded.items() if k.startswith(name + '.')}
    assert sorted(got) == sorted(want) and got['chain'].shape[1] == CASES[name][2] // 20 + 1
    for k in got:
        assert np.array_equal(got[k], want[k]), (name, k)
