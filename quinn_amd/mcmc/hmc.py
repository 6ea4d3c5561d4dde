"""Hamiltonian Monte Carlo for C lock-step chains.

Mirror of the reference's `HMC` (quinn/mcmc/hmc.py:8-70): momentum ~ N(0, I), half kick,
L position steps with L-1 inner kicks, half kick, negate; L+1 gradient evaluations per
proposal -- each of them ONE batched call for all chains.

Build-only extra: `adapt` warm-up steps that tune a per-chain step size and diagonal mass
(`quinn_amd.mcmc.adapt`: the contract the device engine implements too); adapt=0 is the reference's sampler.
"""
import numpy as np

from .adapt import HostAdaptation, TARGET_ACCEPT, check_adapt_args
from .mcmc import MCMCBase


def _kinetic(P):
    # row by row on contiguous 1-D views: the same pairwise summation the reference's
    # np.sum(np.square(p)) performs on its 1-D momentum
    return np.array([np.sum(np.square(P[c])) / 2 for c in range(P.shape[0])])


class AdaptiveLeapfrog(MCMCBase):
    """HMC / MALA with `adapt` warm-up steps: the whitened leapfrog of `quinn_amd.mcmc.adapt` with the per-chain step size
    and scale of a `HostAdaptation`, updated after every warm-up step, frozen afterwards.  Results gain 'epsilon' (C,),
    'mass_scale' (C, p) (None without mass windows) and 'nwarm'."""

    def _init_adapt(self, adapt, target_accept, adapt_mass, kind):
        self.target_accept = TARGET_ACCEPT[kind] if target_accept is None else float(target_accept)
        self.adapt = check_adapt_args(adapt, self.target_accept)
        self.adapt_mass = bool(adapt_mass)
        self._ad = None

    def _run_start(self, cur, nmcmc):
        if self.adapt:
            check_adapt_args(self.adapt, self.target_accept, nmcmc)
            self._ad = HostAdaptation(cur.shape[0], cur.shape[1], self.epsilon, self.adapt, self.target_accept,
                                      self.adapt_mass)

    def _step_done(self, i, cur, mh):
        if self.adapt and i < self.adapt:
            self._ad.update(i + 1, mh, cur)

    def _run_extras(self):
        if not self.adapt:
            return {}
        return {'epsilon': self._ad.eps.copy(), 'mass_scale': None if self._ad.scale is None else self._ad.scale.copy(),
                'nwarm': self.adapt}

    def _whitened_leapfrog(self, current, L):
        C, p = current.shape
        if self._ad is None:                                        # `sampler` called outside `run`
            self._ad = HostAdaptation(C, p, self.epsilon, self.adapt, self.target_accept, self.adapt_mass)
        eps = self._ad.eps[:, None]
        s = 1.0 if self._ad.scale is None else self._ad.scale
        q = current.copy()
        u = np.stack([self.rngs[c].randn(p) for c in range(C)])
        k_cur = _kinetic(u)
        with np.errstate(over="ignore", invalid="ignore"):          # a step size still too large diverges: the MH test rejects
            u += (eps / 2) * s * self._lpg(q)
            q += eps * s * u
            for _ in range(L - 1):
                u += eps * s * self._lpg(q)
                q += eps * s * u
            u += (eps / 2) * s * self._lpg(q)
            return q, k_cur, _kinetic(u)


class HMC(AdaptiveLeapfrog):
    """Args: epsilon (float): leapfrog step size (default 0.05); L (int): leapfrog steps (default 3).
    Build-only: adapt (int, default 0): warm-up steps adapting a per-chain step size from `epsilon` (dual averaging towards
    `target_accept`, default 0.8) and, with adapt_mass (default True), a per-chain diagonal mass matrix."""

    def __init__(self, epsilon=0.05, L=3, adapt=0, target_accept=None, adapt_mass=True):
        super().__init__()
        self.epsilon = epsilon
        self.L = L
        self._init_adapt(adapt, target_accept, adapt_mass, 'hmc')

    def sampler_batch(self, current, imcmc):
        assert self.logPostGrad is not None or self.logPostGradBatch is not None
        if self.adapt:
            return self._whitened_leapfrog(current, self.L)
        C, p = current.shape
        eps = self.epsilon
        q = current.copy()
        mom = np.stack([self.rngs[c].randn(p) for c in range(C)])
        k_cur = _kinetic(mom)
        mom += eps * self._lpg(q) / 2
        for j in range(self.L):
            q += eps * mom
            if j != self.L - 1:
                mom += eps * self._lpg(q)
        mom += eps * self._lpg(q) / 2
        mom = -mom
        return q, k_cur, _kinetic(mom)
