"""Elliptical slice sampling (Murray, Adams & MacKay 2010) with everything resident on the GPU: `DeviceESS`.  Build-only: the
reference has no such sampler.  `quinn_amd.mcmc.ess` states the rule of one iteration and restates it in numpy.

The target is the posterior with the Gaussian weight prior N(0, priorsigma^2 I), which the sampler needs: a step draws a prior
sample nu, and proposes points cur cos(theta) + nu sin(theta) of the ellipse through both, shrinking a bracket of angles around
the current point until the likelihood of a proposal exceeds a slice level.  There is no step size and no warm-up, a step needs
forward calls only, and every step ends on an accepted point ('accrate' is 1 up to the truncation at `max_shrink` proposals,
which is counted).

A step takes a data-dependent number of forward evaluations, so the chains do not run in lock-step: every chain keeps its own
step counter on the device.  One iteration is two launches through the C ABI and nothing else --

    qn_mlp_sse_fwd_parts   SSE parts of every chain's pending proposal
    qn_ess_iter            per chain: shrink the bracket and propose again, or accept, store the row and start the next step

-- and every forward evaluation is one some chain needs (a chain that has made its nmcmc steps idles).  qn_prior_fold is not
launched: the ellipse carries the prior, the slice test sees the likelihood alone.  Iterations are enqueued in blocks of
`block`; after enqueuing block k + 1 the host reads the smallest step counter as of the end of block k (one 8-byte copy into
pinned memory that the GPU never waits for) and stops when it is nmcmc, so at most one block of no-ops is enqueued.

Results: the common keys ('logpost' / 'maxpost' / 'mapparams' in the units of the posterior WITH the prior, as every engine
with `priorsigma` reports them; 'alphas' is 1) plus 'nev' [C, nmcmc + 1] int32 (forward evaluations of each step; row 0 is 0),
'ntrunc' [C] (truncated steps), 'nevals' [C] (= nev summed) and 'accrate' = 1 - ntrunc / nmcmc.  Random streams are keyed by
(seed, the chain's step, global chain id): a chain does not depend on how the chains are split over ranks, engines or groups.

Not here: any prior but the zero-mean isotropic one, tempering (`ladder`), a host engine, graph capture (`use_graph`: the
number of iterations is data dependent).
"""
import numpy as np
import torch

from .. import _lib
from .device_engine import DeviceEngine
from .ess import check_ess_args


class DeviceESS(DeviceEngine):
    """Args: priorsigma (required: the prior's standard deviation), max_shrink (proposals per step before the step is
    truncated and the chain stays; 32 leaves a bracket of ~2 pi / 2^32; narrow likelihoods do
    get there -- watch 'ntrunc' and raise it if truncated steps are not rare), block (iterations enqueued between two looks at the
    chains' step counters), plus the engine's seed / chain0 / groups."""

    _kind = 'ess'

    @classmethod
    def check_params(cls, arch, dtype, nmcmc, priorsigma, max_shrink=32, block=32, use_graph=False, ladder=None, **rest):
        cfg = super().check_params(arch, dtype, nmcmc, priorsigma, **rest)
        if use_graph:
            raise ValueError("DeviceESS with use_graph=True: the number of iterations of a run is data dependent, there is no "
                             "fixed launch sequence to capture; run with use_graph=False")
        if ladder is not None:
            raise ValueError("DeviceESS with ladder: elliptical slice sampling is not tempered (the ellipse is the prior's); "
                             "replica exchange is for sampler='hmc' / 'mala'")
        if cfg['priorsigma'] is None:
            raise ValueError("sampler='ess' needs priorsigma: elliptical slice sampling draws from the Gaussian weight prior "
                             "N(0, priorsigma^2 I); pass fit(..., priorsigma=s) with s > 0")
        cfg['ess'] = check_ess_args(priorsigma, max_shrink, block)
        return cfg

    def __init__(self, op, sigma, priorsigma=None, seed=0, chain0=0, max_shrink=32, block=32, groups=None, use_graph=False,
                 ladder=None):
        ps, self.max_shrink, self.block = self.check_params(op.arch, op.dtype, None, priorsigma, max_shrink=max_shrink, block=block,
                                                            use_graph=use_graph, ladder=ladder)['ess']
        super().__init__(op, sigma, seed, chain0, False, groups, ps)

    def _clone(self, op, chain0):
        return DeviceESS(op, self.sigma, self.priorsigma, self.seed, chain0, self.max_shrink, self.block, groups=1)

    def _extra_keys(self, nmcmc):
        return {'nev': ((nmcmc + 1,), np.int32), 'ntrunc': ((), np.int64), 'nevals': ((), np.int64)}

    def log_prior(self, W):
        """log N(w; 0, priorsigma^2 I) of every row of the device tensor W [C, p]: float64 [C]."""
        s, p = self.priorsigma, W.shape[1]
        return -0.5 * (W * W).sum(dim=1) / s ** 2 - 0.5 * p * np.log(2.0 * np.pi * s ** 2)

    def _iter(self, s, nmcmc):
        """Enqueue one iteration on the current stream: the forward on the pending proposals, then the decision."""
        C, p = s['cur'].shape
        ptr = lambda t: None if t is None else t.data_ptr()
        parts = self.op.sse_parts(s['prop'] if s['prop_op'] is None else s['prop_op'])
        _lib.check(self._L.qn_ess_iter(
            parts.data_ptr(), parts.shape[1], self.sigma, self.priorsigma, self.op.N, self.max_shrink, C, self.chain0, p, nmcmc,
            self.seed, s['cur'].data_ptr(), s['nu'].data_ptr(), s['prop'].data_ptr(), ptr(s['prop_op']), self.op.qdt,
            s['best'].data_ptr(), s['best_lp'].data_ptr(), ptr(s['chain']), s['lps'].data_ptr(), s['nev'].data_ptr(),
            s['sq'].data_ptr(), s['es'].data_ptr(), s['ei'].data_ptr(), s['par'], self._stream()), "qn_ess_iter")
        s['par'] ^= 1

    def _run_gen(self, nmcmc, param_ini, store_chain=True, verbose=False, chain_out=None):
        """The run as a generator: yields after every enqueued block of iterations.  The GPU never waits for the host."""
        nmcmc = int(nmcmc)
        if nmcmc < 1:
            raise ValueError(f"nmcmc = {nmcmc}: a run has >= 1 steps")
        dev, f64 = self.dev, torch.float64
        cur = torch.as_tensor(param_ini, dtype=f64, device=dev).clone().reshape(-1, self.op.p)
        C, p = cur.shape
        f32op = self.op.tdt != f64
        nwg = int(self._L.qn_hmc_parts(p))
        sse0 = self.op.sse(cur)
        lp0 = -(0.5 * sse0 / self.sigma ** 2 + self._const) + self.log_prior(cur)
        s = {'cur': cur, 'nu': torch.empty(C, p, dtype=f64, device=dev), 'prop': torch.empty(C, p, dtype=f64, device=dev),
             'prop_op': torch.empty(C, p, dtype=self.op.tdt, device=dev) if f32op else None,
             'best': cur.clone(), 'best_lp': torch.stack([lp0, lp0]), 'par': 0,
             'chain': (chain_out if chain_out is not None else torch.empty(C, nmcmc + 1, p, dtype=f64, device=dev))
                      if store_chain else None,
             'lps': torch.empty(C, nmcmc + 1, dtype=f64, device=dev),
             'nev': torch.zeros(C, nmcmc + 1, dtype=torch.int32, device=dev),
             'sq': torch.zeros(2, C, nwg, dtype=f64, device=dev),
             'es': torch.zeros(2, C, 6, dtype=f64, device=dev), 'ei': torch.zeros(2, C, 4, dtype=torch.int64, device=dev)}
        if store_chain:
            s['chain'][:, 0] = cur
        s['lps'][:, 0] = lp0
        _lib.check(self._L.qn_ess_begin(
            cur.data_ptr(), sse0.data_ptr(), lp0.data_ptr(), self.sigma, self.priorsigma, C, self.chain0, p, self.seed,
            s['nu'].data_ptr(), s['prop'].data_ptr(), None if s['prop_op'] is None else s['prop_op'].data_ptr(), self.op.qdt,
            s['sq'].data_ptr(), s['es'].data_ptr(), s['ei'].data_ptr(), self._stream()), "qn_ess_begin")
        yield from self._run_blocks(s, nmcmc, nmcmc * self.max_shrink + 2 * self.block, verbose)      # (a step ends within max_shrink iterations)
        par = s['par']
        ei = s['ei'][par]
        ntrunc = ei[:, 2].clone()
        return {'chain': s['chain'], 'mapparams': s['best'], 'maxpost': s['best_lp'][par].clone(),
                'accrate': 1.0 - ntrunc.double() / nmcmc, 'logpost': s['lps'],
                'alphas': torch.ones(C, nmcmc + 1, dtype=f64, device=dev), 'nev': s['nev'], 'ntrunc': ntrunc,
                'nevals': ei[:, 3].clone()}
