"""What the device samplers (`DeviceAMCMC`, `DeviceHMC`, `DeviceMALA`, `DeviceSGHMC`, `DeviceSGLD`) share: the engine's identity
(operator, noise level, optional Gaussian weight prior, seed, global id of the first chain), the per-run state the accept kernel maintains, the result dict, and `run`, which drives a
sampler's step generator (`_run_gen`) for all chains at once or for groups of chains side by side on their own HIP streams."""

import numpy as np
import torch

from .. import _lib
from ..ops import BatchedMLP
from .prior import check_priorsigma, fold_constants


def _drain(gen):
    while True:
        try:
            next(gen)
        except StopIteration as e:
            return e.value


class DeviceEngine:
    """A sampler supplies `_run_gen(nmcmc, param_ini, store_chain, verbose, chain_out=None)` (a generator that yields after
    every enqueued block of steps and returns the result dict), `_ngroups(C)` and `_clone(op, chain0)`."""

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

    def _check_groups(self, nmcmc, C, p):
        """Refuse a run of several groups before any sub-engine exists (default: nothing to refuse)."""

    def _merge_groups(self, out, res, engs):
        """Add to `out` what a sampler returns or keeps beyond the common keys (res: the groups' results, engs: their engines)."""

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
        out = {k: torch.cat([r[k] for r in res]) for k in ('mapparams', 'maxpost', 'accrate', 'logpost', 'alphas')}
        out['chain'] = chain
        self._merge_groups(out, res, engs)
        return out
