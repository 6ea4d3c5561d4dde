"""The No-U-Turn sampler (Hoffman & Gelman 2014; multinomial weights, Betancourt 2017) with everything resident on the GPU:
`DeviceNUTS`.  Build-only: the reference has no such sampler.  `quinn_amd.mcmc.nuts` states the rule of one iteration, restates
it in numpy and pins it to the textbook recursion.

There is no trajectory length: a step doubles its trajectory forwards or backwards until it turns back on itself (or a leaf
diverges, or `max_depth` doublings are made), and takes its next point from the whole trajectory.  What remains to choose is
the step size -- `adapt=K` dual-averages it over the first K steps -- and, optionally, a diagonal mass: pass the `mass_scale`
[C, p] of a `DeviceHMC(adapt=...)` run as it is (its `epsilon` [C] too, but a step size tuned for a short L can be too large for
trajectories of tens of leapfrogs: profiles/nuts.txt).  With `adapt_mass=True` NUTS's own warm-up also finds a per-chain diagonal
mass over the slow windows of `quinn_amd.mcmc.adapt.warmup_schedule(adapt)` (`quinn_amd.mcmc.nuts_adapt` has the contract): the
chains run on their own step counters, so one more launch per iteration, qn_nuts_adapt, looks every chain that has just ended a
warm-up step up in a plan table on the device, dual-averages its step size (restarting at a window end), feeds or closes its
window, and redoes the first half kick and drift of the step that has just started with the new step size and scale.
qn_nuts_iter then runs with adapt = 0; the launch is dropped once the smallest step counter the host has seen is >= adapt.
Without windows (adapt < 20) the run is that of adapt_mass=False.

A step takes a data-dependent number of gradient evaluations, so the chains do not run in lock-step: every chain keeps its own
step counter and its own tree on the device.  One iteration is one leapfrog of every live chain --

    qn_mlp_sse_fwdbwd    SSE and gradient at every chain's pending point
    qn_prior_fold        with `priorsigma`: the Gaussian weight prior into both
    qn_nuts_iter         per chain: complete the leapfrog, test for divergence and U-turns from the checkpoints, then the next
                         leapfrog of the subtree, or merge the subtree and double, or end the step, store the row and start
                         the next step (two launches: reduce; decide and move)
    qn_nuts_adapt        with adapt_mass and windows, during warm-up: step size, moments and scale of the chains that ended a step

-- and every gradient evaluation is one some chain needs (a chain that has made its nmcmc steps idles).  Iterations are enqueued
in blocks of `block`; after enqueuing block k + 1 the host reads the smallest step counter as of the end of block k (one 8-byte
copy into pinned memory that the GPU never waits for) and stops when it is nmcmc.  A step makes at most 2^max_depth - 1 leaves:
the bound is nmcmc (2^max_depth - 1) iterations plus two blocks.

Memory per chain: (15 + 2 max_depth) p float64 of sampler state (tree proposal and gradient, two edges of three vectors, two
momentum sums, the subtree's proposal and gradient, the pending point and momentum, the MAP, 2 max_depth checkpoints) beside the
operator's gradient array and the stored chain.

Results: the common keys, with 'alphas' [C, nmcmc + 1] the acceptance statistic of each step (the mean of min(1, exp(-dE)) over
its leaves; row 0 is 0) and 'accrate' its mean over the steps, plus 'depth' and 'nleap' [C, nmcmc + 1] int32 (doublings started
and leapfrogs of each step), 'ndiv' (divergent steps), 'ntreedepth' (steps stopped by max_depth), 'ngrad' (= nleap summed) [C],
'epsilon' [C] (the step sizes at the end; frozen after warm-up) and 'nwarm' (= adapt); with adapt_mass=True also 'mass_scale'
[C, p], the scale the chains ended with (None without windows).  Random streams are keyed by (seed, the chain's step, global
chain id): a chain does not depend on how the chains are split over ranks, engines or groups.

Not here: tempering (`ladder`), graph capture (`use_graph`: the number of iterations is
data dependent), a host engine, float32 operators, and the extra U-turn checks across adjacent subtrees that Stan added later
(the classic criterion on the tree and on every subtree is made).
"""
import numpy as np
import torch

from .. import _lib
from .device_engine import DeviceEngine
from .adapt import warmup_schedule
from .nuts import check_nuts_args
from .nuts_adapt import plan_table

NES, NEI, NDOT, NWS = 12, 8, 27, 4


class DeviceNUTS(DeviceEngine):
    """Args: epsilon (the step size: a scalar or [C], e.g. an `adapt` run's 'epsilon'), mass_scale (None, or [C, p]: the square
    root of the inverse diagonal mass per chain, e.g. an `adapt` run's 'mass_scale'), max_depth (doublings per step, 1 .. 12),
    adapt (warm-up steps of step-size dual averaging towards target_accept), adapt_mass (True: the warm-up also finds a
    per-chain diagonal mass over the windows of `warmup_schedule(adapt)`, starting from mass_scale or 1; needs adapt > 0),
    block (iterations enqueued between two looks at the chains' step counters), plus the engine's priorsigma / seed / chain0 /
    groups."""

    _kind = 'nuts'

    @classmethod
    def check_params(cls, arch, dtype, nmcmc, priorsigma, epsilon=0.05, max_depth=10, adapt=0, target_accept=0.8, block=32,
                     use_graph=False, ladder=None, adapt_mass=False, **rest):
        cfg = super().check_params(arch, dtype, nmcmc, priorsigma, **rest)
        if use_graph:
            raise ValueError("DeviceNUTS with use_graph=True: the number of iterations of a run is data dependent, there is no "
                             "fixed launch sequence to capture; run with use_graph=False")
        if ladder is not None:
            raise ValueError("DeviceNUTS with ladder: the No-U-Turn sampler is not tempered; replica exchange is for "
                             "sampler='hmc' / 'mala'")
        if dtype != 'float64':
            raise ValueError("DeviceNUTS needs a float64 operator: U-turn tests and energy errors along a trajectory of "
                             "hundreds of leapfrogs are made in float64 (build the operator with dtype='float64')")
        cfg['nuts'] = check_nuts_args(epsilon, max_depth, adapt, target_accept, block, nmcmc)
        if not isinstance(adapt_mass, (bool, np.bool_)):
            raise ValueError(f"adapt_mass = {adapt_mass!r}: True or False")
        if adapt_mass and cfg['nuts'][2] == 0:
            raise ValueError("DeviceNUTS with adapt_mass=True and adapt = 0: the mass windows are part of the warm-up; pass "
                             "adapt=K warm-up steps (windows need K >= 20)")
        cfg['nuts_adapt_mass'] = bool(adapt_mass)
        return cfg

    @classmethod
    def shard_params(cls, sampler_params, lo, hi):
        """The per-chain step sizes [C] and scales [C, p] of all chains: this rank's rows (a scalar step size is everyone's)."""
        return {k: (np.asarray(v, dtype=np.float64)[lo:hi] if k in ('epsilon', 'mass_scale') and np.ndim(v) >= 1 else v)
                for k, v in sampler_params.items()}

    def __init__(self, op, sigma, epsilon=0.05, mass_scale=None, max_depth=10, adapt=0, target_accept=0.8, block=32, seed=0,
                 chain0=0, groups=None, use_graph=False, ladder=None, priorsigma=None, adapt_mass=False):
        if isinstance(epsilon, torch.Tensor):
            epsilon = epsilon.detach().cpu().numpy()
        cfg = self.check_params(op.arch, op.dtype, None, priorsigma, epsilon=epsilon, max_depth=max_depth, adapt=adapt,
                                target_accept=target_accept, block=block, use_graph=use_graph, ladder=ladder, adapt_mass=adapt_mass)
        self.epsilon, self.max_depth, self.adapt, self.target_accept, self.block = cfg['nuts']
        self.adapt_mass = cfg['nuts_adapt_mass']
        self.mass_scale = mass_scale                               # (None, an array or a tensor: checked against C, p in the run)
        super().__init__(op, sigma, seed, chain0, False, groups, priorsigma)

    def _clone(self, op, chain0):
        lo = chain0 - self.chain0
        cut = lambda a: a if a is None or isinstance(a, float) else a[lo:]      # (a group takes its rows from the front)
        return DeviceNUTS(op, self.sigma, cut(self.epsilon), cut(self.mass_scale), self.max_depth, self.adapt, self.target_accept,
                          self.block, self.seed, chain0, groups=1, priorsigma=self.priorsigma, adapt_mass=self.adapt_mass)

    def _extra_keys(self, nmcmc):
        steps, count = ((nmcmc + 1,), np.int32), ((), np.int64)
        keys = {'depth': steps, 'nleap': steps, 'ndiv': count, 'ntreedepth': count, 'ngrad': count, 'epsilon': ((), np.float64),
                'nwarm': self.adapt}
        if self.adapt_mass:
            keys['mass_scale'] = ((self.op.p,), np.float64) if self._windows() else None
        return keys

    def _windows(self):
        """Whether the warm-up has mass windows: adapt_mass and a schedule with a window (adapt >= 20)."""
        return self.adapt_mass and bool(warmup_schedule(self.adapt).ends)

    def _iter(self, s, nmcmc):
        """Enqueue one iteration on the current stream: the gradient at the pending points, the prior, then the decision; in a
        warm-up with windows qn_nuts_iter makes no adaptation of its own (adapt = 0) and, until the slowest chain the host has
        seen (s['tmin'], one block late) has left the warm-up, qn_nuts_adapt follows it."""
        C, p = s['cur'].shape
        self.op.sse_grad(s['q'], out=(s['sse'], s['gq']))
        if self._prior is not None:
            self.op.prior_fold(s['q'], *self._prior, sse=s['sse'], grad=s['gq'])
        ptr = lambda t: None if t is None else t.data_ptr()
        _lib.check(self._L.qn_nuts_iter(
            s['sse'].data_ptr(), s['gq'].data_ptr(), ptr(s['scale']), self.sigma, self.op.N, self.max_depth,
            0 if 'ws' in s else self.adapt,
            self.target_accept, C, self.chain0, p, nmcmc, self.seed, *(s[k].data_ptr() for k in self._VEC),
            s['best'].data_ptr(), s['best_lp'].data_ptr(), ptr(s['chain']), s['lps'].data_ptr(), s['alphas'].data_ptr(),
            s['depth'].data_ptr(), s['nleap'].data_ptr(), s['dots'].data_ptr(), s['zz'].data_ptr(), s['es'].data_ptr(),
            s['ei'].data_ptr(), s['par'], self._stream()), "qn_nuts_iter")
        if 'ws' in s and s.get('tmin', 0) < self.adapt:
            _lib.check(self._L.qn_nuts_adapt(
                s['cur'].data_ptr(), s['alphas'].data_ptr(), nmcmc, self.adapt, self.target_accept, s['plan'].data_ptr(),
                s['es'].data_ptr(), s['ei'].data_ptr(), s['par'], C, p, self.sigma, s['ql'].data_ptr(), s['ul'].data_ptr(),
                s['gl'].data_ptr(), s['q'].data_ptr(), s['u'].data_ptr(), s['ws'].data_ptr(), s['mean'].data_ptr(),
                s['m2'].data_ptr(), s['scale'].data_ptr(), self._stream()), "qn_nuts_adapt")
        s['par'] ^= 1

    _VEC = ('cur', 'gcur', 'ql', 'ul', 'gl', 'qr', 'ur', 'gr', 'rho', 'q', 'u', 'rho_sub', 'sub_q', 'sub_g', 'ck_u', 'ck_rho')

    def _run_gen(self, nmcmc, param_ini, store_chain=True, verbose=False, chain_out=None):
        """The run as a generator: yields after every enqueued block of iterations.  The GPU never waits for the host."""
        nmcmc = int(nmcmc)
        if nmcmc < 1:
            raise ValueError(f"nmcmc = {nmcmc}: a run has >= 1 steps")
        check_nuts_args(self.epsilon, self.max_depth, self.adapt, self.target_accept, self.block, nmcmc)
        dev, f64 = self.dev, torch.float64
        cur = torch.as_tensor(param_ini, dtype=f64, device=dev).clone().reshape(-1, self.op.p)
        C, p = cur.shape
        eps0 = torch.as_tensor(self.epsilon, dtype=f64, device=dev).reshape(-1)
        if np.ndim(self.epsilon) == 0:
            eps0 = eps0.expand(C)
        if eps0.shape[0] < C:
            raise ValueError(f"epsilon has {eps0.shape[0]} entries for {C} chains")
        eps0 = eps0[:C].contiguous()
        scale = None
        if self.mass_scale is not None:
            scale = torch.as_tensor(self.mass_scale, dtype=f64, device=dev).reshape(-1, p)
            if scale.shape[0] < C:
                raise ValueError(f"mass_scale has {scale.shape[0]} rows for {C} chains")
            scale = scale[:C].contiguous()
            if not bool((torch.isfinite(scale) & (scale > 0)).all()):
                raise ValueError("mass_scale: every entry must be > 0 and finite")
        nwg = int(self._L.qn_hmc_parts(p))
        sse0, g0 = self.op.sse_grad(cur)
        if self._prior is not None:
            self.op.prior_fold(cur, *self._prior, sse=sse0, grad=g0)
        lp0 = -(0.5 * sse0 / self.sigma ** 2 + self._const)
        vec = lambda: torch.empty(C, p, dtype=f64, device=dev)
        s = {k: vec() for k in self._VEC[2:14]}
        s.update({'cur': cur, 'gcur': g0.clone(), 'scale': scale, 'best': cur.clone(), 'par': 0,
                  'ck_u': torch.empty(C, self.max_depth, p, dtype=f64, device=dev),
                  'ck_rho': torch.empty(C, self.max_depth, p, dtype=f64, device=dev),
                  'gq': torch.empty(C, p, dtype=f64, device=dev), 'sse': torch.empty(C, dtype=f64, device=dev),
                  'best_lp': torch.zeros(2, C, dtype=f64, device=dev),
                  'chain': (chain_out if chain_out is not None else torch.empty(C, nmcmc + 1, p, dtype=f64, device=dev))
                           if store_chain else None,
                  'lps': torch.empty(C, nmcmc + 1, dtype=f64, device=dev),
                  'alphas': torch.zeros(C, nmcmc + 1, dtype=f64, device=dev),
                  'depth': torch.zeros(C, nmcmc + 1, dtype=torch.int32, device=dev),
                  'nleap': torch.zeros(C, nmcmc + 1, dtype=torch.int32, device=dev),
                  'dots': torch.zeros(C, nwg, NDOT, dtype=f64, device=dev), 'zz': torch.zeros(2, C, nwg, dtype=f64, device=dev),
                  'es': torch.zeros(2, C, NES, dtype=f64, device=dev), 'ei': torch.zeros(2, C, NEI, dtype=torch.int64, device=dev)})
        if self._windows():                                        # the warm-up's own state: a writable scale, the plan, ws, moments
            s['scale'] = scale = torch.ones(C, p, dtype=f64, device=dev) if scale is None else scale.clone()
            s['plan'] = torch.as_tensor(plan_table(self.adapt), device=dev)
            s['ws'] = torch.zeros(2, C, NWS, dtype=f64, device=dev)
            s['ws'][0, :, 0], s['ws'][0, :, 3] = torch.log(10 * eps0), eps0
            s['mean'], s['m2'] = torch.zeros(C, p, dtype=f64, device=dev), torch.zeros(C, p, dtype=f64, device=dev)
        if store_chain:
            s['chain'][:, 0] = cur
        s['lps'][:, 0] = lp0
        ptr = lambda t: None if t is None else t.data_ptr()
        _lib.check(self._L.qn_nuts_begin(
            sse0.data_ptr(), eps0.data_ptr(), ptr(scale), self.sigma, self.op.N, C, self.chain0, p, self.seed,
            *(s[k].data_ptr() for k in self._VEC[:11]), s['zz'].data_ptr(), s['best_lp'].data_ptr(), s['es'].data_ptr(),
            s['ei'].data_ptr(), self._stream()), "qn_nuts_begin")
        yield from self._run_blocks(s, nmcmc, nmcmc * (2 ** self.max_depth - 1) + 2 * self.block, verbose)      # (a step: <= 2^max_depth - 1)
        par = s['par']
        es, ei = s['es'][par], s['ei'][par]
        out = {'chain': s['chain'], 'mapparams': s['best'], 'maxpost': s['best_lp'][par].clone(),
               'accrate': s['alphas'][:, 1:].mean(dim=1), 'logpost': s['lps'], 'alphas': s['alphas'], 'depth': s['depth'],
               'nleap': s['nleap'], 'ndiv': ei[:, 5].clone(), 'ntreedepth': ei[:, 6].clone(), 'ngrad': ei[:, 7].clone(),
               'epsilon': es[:, 0].clone(), 'nwarm': self.adapt}
        if self.adapt_mass:
            out['mass_scale'] = s['scale'] if 'ws' in s else None
        return out
