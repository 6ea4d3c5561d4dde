"""Metropolis-adjusted Langevin for C lock-step chains.

Mirror of the reference's `MALA` (quinn/mcmc/mala.py:8-53): one Langevin step, two
gradient evaluations per proposal (each ONE batched call).  Unlike the reference
(where `sampler='mala'` falls through NN_MCMC.fit's dispatch, nn_mcmc.py:130-135, and
raises UnboundLocalError) `NN_MCMC.fit(sampler='mala')` reaches this class.
"""
import numpy as np

from .hmc import AdaptiveLeapfrog, _kinetic


class MALA(AdaptiveLeapfrog):
    """Args: epsilon (float): step size (default 0.05).
    Build-only: adapt / target_accept (default 0.574) / adapt_mass as `HMC`: MALA is the leapfrog with L = 1."""

    def __init__(self, epsilon=0.05, adapt=0, target_accept=None, adapt_mass=True):
        super().__init__()
        self.epsilon = epsilon
        self._init_adapt(adapt, target_accept, adapt_mass, 'mala')

    def sampler_batch(self, current, imcmc):
        assert self.logPostGrad is not None or self.logPostGradBatch is not None
        if self.adapt:
            return self._whitened_leapfrog(current, 1)
        C, p = current.shape
        eps = self.epsilon
        q = current.copy()
        mom = np.stack([self.rngs[c].randn(p) for c in range(C)])
        g_cur = self._lpg(current)
        q += 0.5 * eps ** 2 * g_cur + eps * mom
        g_prop = self._lpg(q)
        k_cur = _kinetic(mom)
        mom += eps * (g_cur + g_prop) / 2
        return q, k_cur, _kinetic(mom)
