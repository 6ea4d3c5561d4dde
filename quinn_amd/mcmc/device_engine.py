"""What the device samplers (`DeviceAMCMC`, `DeviceHMC`, `DeviceMALA`, `DeviceSGHMC`, `DeviceSGLD`) share: the engine's identity
(operator, noise level, optional Gaussian weight prior, seed, global id of the first chain), the per-run state the accept kernel maintains, the result dict, and `run`, which drives a
sampler's step generator (`_run_gen`) for all chains at once or for groups of chains side by side on their own HIP streams."""

import numpy as np
import torch

from .. import _lib, parallel
from ..ops import BatchedMLP
from .prior import check_priorsigma, fold_constants


def priors_refusal(name, sampler, engine):
    """The text that refuses `hyperprior` / `noiseprior` (name) everywhere but on the device HMC / MALA engines."""
    return f"{name} runs with sampler='hmc' | 'mala' and engine='device' only (got sampler={sampler!r}, engine={engine!r})"


def _drain(gen):
    while True:
        try:
            next(gen)
        except StopIteration as e:
            return e.value


class DeviceEngine:
    """A sampler supplies `_run_gen(nmcmc, param_ini, store_chain, verbose, chain_out=None)` (a generator that yields after
    every enqueued block of steps and returns the result dict) and `_clone(op, chain0)`; it states its refusal rules in
    `check_params` and what its result holds beyond the common keys in `_extra_keys`."""
    _kind = None                           # the name `NN_MCMC.fit(sampler=...)` knows the engine by

    @classmethod
    def check_params(cls, arch, dtype, nmcmc, priorsigma, hyperprior=None, noiseprior=None, **rest):
        """Every refusal that host values decide, stated once: the constructor calls it with the operator's architecture and
        dtype ('float64' | 'float32'), `NN_MCMC.fit` with the solver's, before any device is touched (no library, no operator,
        no torch.cuda call here or in an override).  nmcmc: the run's steps (None: not known yet); the keywords: the sampler's
        parameters under the constructor's names, and nchains / chain0 where the caller knows them (rest: those no rule
        reads).  Returns the normalised settings the constructor keeps, as a dict."""
        for name, val in (('hyperprior', hyperprior), ('noiseprior', noiseprior)):
            if val is not None:
                raise ValueError(priors_refusal(name, cls._kind, 'device'))
        return {'priorsigma': check_priorsigma(priorsigma)}

    @classmethod
    def shard_params(cls, sampler_params, lo, hi):
        """sampler_params of all chains -> those of the chains [lo, hi) of one rank (default: nothing is per chain)."""
        return sampler_params

    def __init__(self, op: BatchedMLP, sigma, seed, chain0, use_graph, groups, priorsigma=None):
        self.op, self.sigma = op, float(sigma)
        # isotropic Gaussian weight prior N(0, priorsigma^2 I) (`quinn_amd.mcmc.prior`): one qn_prior_fold launch behind every
        # forward / gradient call puts it into the SSE and d SSE / d W the sampler kernels read.  None: no prior, no launch
        self.priorsigma = check_priorsigma(priorsigma)
        self._prior = None if self.priorsigma is None else fold_constants(self.sigma, self.priorsigma, op.p)
        self.dev = op.device
        self.seed = int(seed) & (2 ** 63 - 1)
        self.chain0 = int(chain0)          # global id of this engine's first chain (random streams are keyed by it)
        self.use_graph = bool(use_graph)
        # groups > 1: the chains run as that many independent groups, each on its own HIP stream, enqueued block by block from
        # this one host thread.  A group's launches split a chain's rows as the launch of all chains would
        # (qn_mlp_desc_set_plan_batch), so the chains do not depend on the number of groups, bit for bit
        self.groups = None if groups is None else max(1, int(groups))
        self._subs = None
        self.last_iters = None             # (diagnostics, `_run_blocks`: iterations enqueued by the last run, and how many were needed)
        self._L = _lib.lib()
        n = op.N
        self._const = (n / 2) * np.log(2 * np.pi) + n * np.log(self.sigma)

    def _stream(self):
        return _lib.stream(self.dev)

    @staticmethod
    def _step_ptr(s):
        """Pointer to the CURRENT slot of the double-buffered device step counter (include/quinn_amd.h)."""
        return s['step'].data_ptr() + 8 * s['par']

    def _new_state(self, cur, sse0, nmcmc, store_chain, chain_out):
        """The state every accept kernel maintains, from the start points cur [C, p] and their SSE, with row 0 of the history
        written.  The per-chain scalars are double-buffered by step parity ([2, C]; slot `par` is current)."""
        dev, f64 = self.dev, torch.float64
        C, p = cur.shape
        cur_lp = -(0.5 * sse0 / self.sigma ** 2 + self._const)
        s = {'cur': cur, 'cur_lp': torch.stack([cur_lp, cur_lp]), 'best': cur.clone(),
             'best_lp': torch.stack([cur_lp, cur_lp]), 'par': 0,
             'chain': (chain_out if chain_out is not None else torch.empty(C, nmcmc + 1, p, dtype=f64, device=dev))
                      if store_chain else None,
             'lps': torch.empty(C, nmcmc + 1, dtype=f64, device=dev),
             'alphas': torch.zeros(C, nmcmc + 1, dtype=f64, device=dev),
             'nacc': torch.zeros(C, dtype=torch.int64, device=dev),
             'step': torch.zeros(2, dtype=torch.int64, device=dev)}
        if store_chain:
            s['chain'][:, 0] = cur
        s['lps'][:, 0] = cur_lp
        return s

    @staticmethod
    def _results(s, nmcmc):
        return {'chain': s['chain'], 'mapparams': s['best'], 'maxpost': s['best_lp'][s['par']].clone(),
                'accrate': s['nacc'].double() / max(nmcmc, 1), 'logpost': s['lps'], 'alphas': s['alphas']}

    def _run_blocks(self, s, nmcmc, bound, verbose):
        """The loop of the engines whose chains advance asynchronously (`DeviceESS`, `DeviceNUTS`), as a generator: `_iter` is
        enqueued in blocks of `block` iterations, with a yield after every block, until every chain has made nmcmc steps
        (bound: the iterations that cannot be exceeded).  Sets `last_iters` = (iterations enqueued, iterations needed)."""
        dev = self.dev
        # the smallest step counter after each block: reduced on the device, copied into pinned memory behind the block, and
        # looked at one block late -- when the next block is already enqueued
        tmin_dev = torch.empty(2, dtype=torch.int64, device=dev)
        tmin_host = torch.zeros(2, dtype=torch.int64).pin_memory()
        events = [torch.cuda.Event(), torch.cuda.Event()]
        k = 0
        while True:
            for _ in range(self.block):
                self._iter(s, nmcmc)
            torch.amin(s['ei'][s['par'], :, 0], dim=0, out=tmin_dev[k & 1])
            tmin_host[k & 1].copy_(tmin_dev[k & 1], non_blocking=True)
            events[k & 1].record(torch.cuda.current_stream(dev))
            k += 1
            yield
            if k >= 2:
                events[k & 1].synchronize()                        # block k - 2 (0-based): block k - 1 is already enqueued
                tmin = s['tmin'] = int(tmin_host[k & 1])            # (`_iter` may read it: what the host knows of the slowest chain)
                if verbose:
                    print('%d iterations enqueued, slowest chain at step %d / %d' % (k * self.block, tmin, nmcmc))
                if tmin >= nmcmc:
                    break
            if k * self.block >= bound:                            # (cannot happen: the bound is on the iterations of a step)
                raise _lib.QuinnAmdError(f"{type(self).__name__}: the chains did not finish within {bound} iterations")
        self.last_iters = (k * self.block, (k - 1) * self.block)

    def _ngroups(self, C):
        return 1 if self.groups is None else min(self.groups, C)

    def _check_groups(self, nmcmc, C, p):
        """Refuse a run of several groups before any sub-engine exists (default: nothing to refuse)."""

    def _extra_keys(self, nmcmc):
        """What the result of a run of nmcmc steps holds beyond the six common keys, in the order `_run_gen` adds it:
        {key: (trailing shape, numpy dtype)} for an array with one row per chain, {key: value} for a scalar or None that is the
        same for all chains.  `_run_gen` stays the authority on values; keys, dtypes and shapes are stated here alone."""
        return {}

    def empty_results(self, nmcmc):
        """The result of a rank that owns no chain: the keys, dtypes and trailing shapes of a run's result, no rows."""
        out = parallel.empty_results(nmcmc, self.op.p)
        out.update((k, np.zeros((0,) + v[0], dtype=v[1]) if isinstance(v, tuple) else v)
                   for k, v in self._extra_keys(nmcmc).items())
        return out

    def _merge_groups(self, out, res, engs, nmcmc):
        """Add to `out` what a sampler returns beyond the common keys (res: the groups' results, engs: their engines): the
        per-chain arrays concatenated, the scalars passed through; and keep the groups' `last_iters`.  An override calls this."""
        for k, v in self._extra_keys(nmcmc).items():
            out[k] = torch.cat([r[k] for r in res]) if isinstance(v, tuple) else res[0][k]
        self.last_iters = [e.last_iters for e in engs]

    def run(self, nmcmc, param_ini, store_chain=True, verbose=False):
        ini = torch.as_tensor(np.asarray(param_ini), dtype=torch.float64, device=self.dev).reshape(-1, self.op.p)
        C, p = ini.shape
        G = self._ngroups(C)
        if G <= 1:
            return _drain(self._run_gen(nmcmc, ini, store_chain, verbose))
        # ---- several groups of chains side by side
        bounds = [C * g // G for g in range(G + 1)]
        self._check_groups(nmcmc, C, p)
        if self._subs is None or [e.chain0 - self.chain0 for e in self._subs[0]] != bounds[:-1]:
            op = self.op
            engs = [self._clone(BatchedMLP(op.arch, op.X, op.Y, device=op.device, dtype=op.dtype), self.chain0 + bounds[g])
                    for g in range(G)]
            for e in engs:
                # a group's launches split every chain's rows as the launch of all C chains does: each chain's SSE is summed in
                # the same order, so the chains are those of groups = 1 bit for bit (include/quinn_amd.h)
                e.op.set_plan_batch(max(C, op.set_plan_batch(-1)))
                path = op.set_path(_lib.PATH_AUTO)                            # (the kernel family forced on the parent, if any)
                op.set_path(path)
                e.op.set_path(path)
            self._subs = (engs, [torch.cuda.Stream(device=self.dev) for _ in range(G)])
        engs, streams = self._subs
        chain = torch.empty(C, nmcmc + 1, p, dtype=torch.float64, device=self.dev) if store_chain else None
        gens = [engs[g]._run_gen(nmcmc, ini[bounds[g]:bounds[g + 1]], store_chain, verbose and g == 0,
                                 chain_out=None if chain is None else chain[bounds[g]:bounds[g + 1]]) for g in range(G)]
        main = torch.cuda.current_stream(self.dev)
        for st in streams:
            st.wait_stream(main)
        res, live = [None] * G, list(range(G))
        while live:
            for g in list(live):
                with torch.cuda.stream(streams[g]):
                    try:
                        next(gens[g])
                    except StopIteration as e:
                        res[g] = e.value
                        live.remove(g)
        for st in streams:
            main.wait_stream(st)
        out = {'chain': chain}               # (the keys in the order of `_results`: `gather_results` pairs the ranks' arrays by it)
        out.update((k, torch.cat([r[k] for r in res])) for k in ('mapparams', 'maxpost', 'accrate', 'logpost', 'alphas'))
        self._merge_groups(out, res, engs, nmcmc)
        return out
