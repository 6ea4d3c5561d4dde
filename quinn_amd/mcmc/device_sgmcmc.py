"""Stochastic-gradient MCMC with states, momenta, minibatch rows and history resident on the GPU: `DeviceSGHMC` (Chen et al.
2014) and `DeviceSGLD` (Welling & Teh 2011; SGHMC with alpha = 1), optionally with the cyclical step size of Zhang et al. 2020.
Build-only: the reference has no such sampler.  `quinn_amd.mcmc.sgmcmc` states the update and restates it in numpy.

Every other sampler of this package pays for the full dataset on every step; these evaluate the gradient on `batch` rows that
each chain draws for itself, on the device.  One inner step is two launches through the C ABI and nothing else -- no torch op,
no host synchronisation:

    qn_mlp_sse_fwdbwd   SSE and gradient of every chain on its own rows (row_idx = the current half of rows [2, C, Nb])
    qn_sg_step          position / momentum update with in-kernel Philox noise, log-posterior trace of the incoming state,
                        history row of the outgoing one, the NEXT step's rows into the other half, device step counter

`nmcmc` is the number of stored rows after row 0; a run makes nmcmc * thin inner steps and ends with one more gradient call
and a flagged qn_sg_step that records the last row's log-posterior.  There is no accept test: 'accrate' and 'alphas' are 1.
'logpost' is the MINIBATCH estimate -((N / Nb) SSE_b / (2 sigma^2) + const) of each stored state on the rows of the step that
consumes it (exact with batch=None); 'mapparams' / 'maxpost' maximise that estimate over the stored states.  Random streams
are keyed by (seed, inner step, global chain id): a chain's rows and noise do not depend on how the chains are split over
ranks, engines or groups.  With `use_graph=True` two steps (parity 0 and 1) are captured once in a HIP graph and replayed; the
step size schedule reads the device step counter, so it survives the replay."""
import numpy as np
import torch

from .. import _lib
from .device_engine import DeviceEngine
from .prior import fold_constants
from .sgmcmc import SCHEDULES, check_sg_args


class DeviceSGHMC(DeviceEngine):
    """Args: eta (step size; in the units of SGLD's eta: the position moves by -eta grad U per step), alpha (friction in
    (0, 1], default 0.1; 1 is SGLD), batch (rows per chain and step, drawn with replacement; None: all rows in order, a
    deterministic gradient), thin (every thin-th state is stored), schedule ('constant' | 'cyclic'), cycles and explore_frac
    (cyclic: number of cosine cycles over the run, and the head of each cycle that runs without noise), temperature (1: the
    posterior; 0: no noise), plus the engine's seed / chain0 / use_graph / groups and priorsigma (None: no prior; s: the Gaussian
    weight prior N(0, s^2 I), folded into every minibatch call's SSE and gradient with the constants times Nb / N, so that the
    update's N / Nb leaves it unscaled: the prior is exact, only the likelihood is estimated)."""

    _kind = 'sghmc'

    @classmethod
    def check_params(cls, arch, dtype, nmcmc, priorsigma, eta=1e-5, alpha=0.1, batch=None, thin=1, schedule='constant', cycles=1,
                     explore_frac=0.0, temperature=1.0, **rest):
        cfg = super().check_params(arch, dtype, nmcmc, priorsigma, **rest)
        check_sg_args(eta, alpha, batch, thin, schedule, cycles, explore_frac, temperature, nmcmc)
        return cfg

    def __init__(self, op, sigma, eta=1e-5, alpha=0.1, batch=None, thin=1, schedule='constant', cycles=1, explore_frac=0.0,
                 temperature=1.0, seed=0, chain0=0, use_graph=False, groups=None, priorsigma=None):
        self.check_params(op.arch, op.dtype, None, priorsigma, eta=eta, alpha=alpha, batch=batch, thin=thin, schedule=schedule,
                          cycles=cycles, explore_frac=explore_frac, temperature=temperature)
        self.eta, self.alpha = float(eta), float(alpha)
        self.batch = None if batch is None else int(batch)
        self.thin, self.schedule, self.cycles = int(thin), schedule, int(cycles)
        self.explore_frac, self.temperature = float(explore_frac), float(temperature)
        super().__init__(op, sigma, seed, chain0, use_graph, groups, priorsigma)

    def _clone(self, op, chain0):
        return DeviceSGHMC(op, self.sigma, self.eta, self.alpha, self.batch, self.thin, self.schedule, self.cycles,
                           self.explore_frac, self.temperature, self.seed, chain0, self.use_graph, groups=1,
                           priorsigma=self.priorsigma)

    def _step(self, s, nmcmc, final=False):
        """Enqueue one inner step on the current stream: the gradient on the rows of slot s['par'], then the update (final: the
        last row's log-posterior only)."""
        C, p = s['theta'].shape
        par = s['par']
        ptr = lambda t: None if t is None else t.data_ptr()
        rows = s['rows']
        self.op.sse_grad(s['theta'] if s['thop'] is None else s['thop'], row_idx=None if rows is None else rows[par],
                         out=(s['sse'], s['g']))
        if s['prior'] is not None:                  # (lam, c0) x Nb / N: the update's N / Nb leaves the prior unscaled
            self.op.prior_fold(s['theta'], *s['prior'], sse=s['sse'], grad=s['g'])
        _lib.check(self._L.qn_sg_step(
            s['theta'].data_ptr(), ptr(s['v']), s['g'].data_ptr(), self.op.qdt, s['sse'].data_ptr(), self.sigma, self.op.N,
            s['Nb'], self.eta, self.alpha, self.temperature, SCHEDULES.index(self.schedule), s['K'] or 0, self.explore_frac,
            self.thin, int(final), C, self.chain0, p, nmcmc, self.seed, ptr(s['thop']), s['best'].data_ptr(),
            s['best_lp'].data_ptr(), ptr(s['chain']), s['lps'].data_ptr(), ptr(rows), s['step'].data_ptr(), par,
            self._stream()), "qn_sg_step")
        s['par'] ^= 1

    def _run_gen(self, nmcmc, param_ini, store_chain=True, verbose=False, chain_out=None):
        """The run as a generator: yields after every enqueued step (pair of steps under a graph); nothing is awaited."""
        K = check_sg_args(self.eta, self.alpha, self.batch, self.thin, self.schedule, self.cycles, self.explore_frac,
                          self.temperature, nmcmc)
        dev, f64 = self.dev, torch.float64
        cur = torch.as_tensor(param_ini, dtype=f64, device=dev).clone().reshape(-1, self.op.p)
        C, p = cur.shape
        f32op = self.op.tdt != f64
        Nb = self.op.N if self.batch is None else self.batch
        s = {'theta': cur, 'v': None if self.alpha == 1.0 else torch.zeros(C, p, dtype=f64, device=dev),
             'thop': cur.to(self.op.tdt) if f32op else None,
             'g': torch.empty(C, p, dtype=self.op.tdt, device=dev), 'sse': torch.empty(C, dtype=f64, device=dev),
             'best': cur.clone(), 'best_lp': torch.full((2, C), -np.inf, dtype=f64, device=dev),
             'chain': (chain_out if chain_out is not None else torch.empty(C, nmcmc + 1, p, dtype=f64, device=dev))
                      if store_chain else None,
             'lps': torch.empty(C, nmcmc + 1, dtype=f64, device=dev),
             'rows': None if self.batch is None else torch.empty(2, C, Nb, dtype=torch.int32, device=dev),
             'step': torch.zeros(2, dtype=torch.int64, device=dev), 'par': 0, 'Nb': Nb, 'K': K,
             'prior': None if self.priorsigma is None else fold_constants(self.sigma, self.priorsigma, p, self.op.N, Nb)}
        if store_chain:
            s['chain'][:, 0] = cur
        if s['rows'] is not None:                                  # rows of step 0; every later step draws its successor's
            _lib.check(self._L.qn_sg_rows(s['rows'].data_ptr(), C, Nb, self.op.N, self.chain0, self.seed, s['step'].data_ptr(),
                                          0, self._stream()), "qn_sg_rows")
        total, i = nmcmc * self.thin, 0
        step = self._step
        if self.use_graph and total >= 4:
            # two steps (parity 0 and 1) captured once; warm the kernels up on a side stream first (torch's capture rule)
            side = torch.cuda.Stream(device=dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                step(s, nmcmc)
                step(s, nmcmc)
            torch.cuda.current_stream(dev).wait_stream(side)
            i += 2
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                step(s, nmcmc)
                step(s, nmcmc)
            i += 2                                         # (capture does not run the kernels: replay once for steps 2, 3)
            graph.replay()
            yield
            while i + 2 <= total:
                graph.replay()
                i += 2
                yield
        while i < total:
            step(s, nmcmc)
            i += 1
            yield
            if verbose and total >= 10 and i % (total // 10) == 0:
                print('%d / %d inner steps enqueued' % (i, total))
        step(s, nmcmc, final=True)
        ones = torch.ones(C, nmcmc + 1, dtype=f64, device=dev)
        return {'chain': s['chain'], 'mapparams': s['best'], 'maxpost': s['best_lp'][s['par']].clone(),
                'accrate': torch.ones(C, dtype=f64, device=dev), 'logpost': s['lps'], 'alphas': ones}


class DeviceSGLD(DeviceSGHMC):
    """Stochastic-gradient Langevin dynamics: `DeviceSGHMC` with alpha = 1 (no momentum array)."""
    _kind = 'sgld'

    def __init__(self, op, sigma, eta=1e-5, batch=None, thin=1, schedule='constant', cycles=1, explore_frac=0.0,
                 temperature=1.0, seed=0, chain0=0, use_graph=False, groups=None, priorsigma=None):
        super().__init__(op, sigma, eta=eta, alpha=1.0, batch=batch, thin=thin, schedule=schedule, cycles=cycles,
                         explore_frac=explore_frac, temperature=temperature, seed=seed, chain0=chain0, use_graph=use_graph,
                         groups=groups, priorsigma=priorsigma)
