"""MCMC wrapper around a user MLP, all chains' log-posteriors evaluated in one launch.

Mirror of the reference's `NN_MCMC` (quinn/solvers/nn_mcmc.py:15-200): same constructor,
`fit` / `logpost` / `logpostgrad` / `predict_*` signatures and attributes (`samples`,
`cmode`, `pdim`, `lpinfo`).  Build-only keyword extras (defaults = reference behaviour):
`nchains`, `seeds` on `fit`; `device`, `dtype` on the constructor.

logpost(w) = -[ 0.5*SSE(w)/sigma^2 + (N/2) log 2pi + N log sigma ]   (no prior by default, as
nn_mcmc.py:64 -> losses.py:197-200); SSE and dSSE/dw come from the HIP kernels, the scalar
tail is applied here in float64.  `fit(..., priorsigma=s)` (build-only) adds the isotropic Gaussian weight prior
log N(w; 0, s^2 I), normaliser included, on every engine (`quinn_amd.mcmc.prior`).  With gradient observations (`fit(..., gtrn=, gradnoise=)`) a second Gaussian
likelihood term on the input Jacobian is added (host engine; `BatchedMLP.sobolev`).
"""
import copy
import sys

import numpy as np
import torch
from scipy.optimize import minimize

from ..mcmc.admcmc import AMCMC
from ..mcmc.hmc import HMC
from ..mcmc.mala import MALA
from ..mcmc.device_amcmc import DeviceAMCMC
from ..mcmc.device_engine import priors_refusal
from ..mcmc.device_hmc import DeviceHMC
from ..mcmc.device_mala import DeviceMALA
from ..mcmc.device_sgmcmc import DeviceSGHMC, DeviceSGLD
from ..mcmc.device_ess import DeviceESS
from ..mcmc.device_nuts import DeviceNUTS
from ..mcmc import diagnostics as diag
from ..mcmc import rankdiag
from ..mcmc.tempering import check_whole_ladders
from ..mcmc.prior import check_priorsigma, grad_log_prior, log_prior
from .. import scoring
from ..ops import BatchedMLP, neg_log_post_from_sse, check_gradloss_args
from ..parallel import dist_info, gather_results, run_chains_sharded, shard_bounds
from .quinn import QUiNNBase

# fit(engine='device'): sampler -> class (its `check_params` refuses what it cannot run, before any device is touched)
DEVICE_ENGINES = {'amcmc': DeviceAMCMC, 'hmc': DeviceHMC, 'mala': DeviceMALA, 'sgld': DeviceSGLD, 'sghmc': DeviceSGHMC,
                  'ess': DeviceESS, 'nuts': DeviceNUTS}
# stochastic-gradient samplers, elliptical slice sampling, the No-U-Turn sampler: no host counterpart
DEVICE_ONLY = ('sgld', 'sghmc', 'ess', 'nuts')
# fit(engine='host'): sampler -> (class, whether it takes the gradient hook)
HOST_SAMPLERS = {'amcmc': (AMCMC, False), 'hmc': (HMC, True), 'mala': (MALA, True)}


def _rank_keys(stats):
    """The dict of `rankdiag.rank_stats` as it is merged into a diagnostics dict: the figures under their own names, the plan
    (n_draws, nh, stride, t0) under rank_*, so that the batch plan's n_draws and t0 stay what they were."""
    return {(f"rank_{k}" if k in ("n_draws", "nh", "stride", "t0") else k): v for k, v in stats.items()}


class NN_MCMC(QUiNNBase):
    """Attributes: samples `(nmcmc+1, p)` (or `(C, nmcmc+1, p)` for C chains), cmode (MAP
    weights), pdim, lpinfo, verbose."""

    def __init__(self, nnmodel, verbose=True, device=None, dtype="float64", kernels="auto"):
        """kernels (build-only extra; the reference has no counterpart): 'auto' -- the fastest kernel family for the network's
        shape; for 64 / 128 / 256-wide tanh networks in float64 those are the sliced int8-product kernels, whose operands are
        rounded to 2^-47 of their row / activation scale (a norm-wise 47-bit bound: ~1e-14 .. 1e-13 on log-posteriors and
        gradients of ordinary networks, where float64 rounding gives ~1e-16).  'float64' -- plain float64 arithmetic
        throughout (the float64-MFMA fused kernels where they apply, the layer-wise float64 kernels otherwise): what the
        reference's torch CPU path computes, up to summation order."""
        super().__init__(nnmodel, device=device, dtype=dtype)
        if kernels not in ("auto", "float64"):
            raise ValueError("kernels must be 'auto' or 'float64'")
        self.kernels = kernels
        self.verbose = verbose
        self.pdim = sum(p.numel() for p in self.nnmodel.parameters())
        print("Number of parameters:", self.pdim)
        if self.verbose:
            self.print_params(names_only=True)
        self.samples = None
        self.cmode = None
        self.lpinfo = {}
        self.diagnostics = None
        self._op = None
        self._op_key = None

    # -- device operator bound to lpinfo's dataset -----------------------------------------
    def _operator(self, lpinfo):
        # the cached operator belongs to these very objects (kept referenced here, compared with `is`: an id() alone
        # can be recycled by a new array after the old one is freed)
        key = (lpinfo['xd'], lpinfo['yd'], lpinfo.get('gd'))
        if self._op is None or any(a is not b for a, b in zip(self._op_key, key)):
            xd = np.asarray(lpinfo['xd'], dtype=np.float64)
            yd = np.asarray(lpinfo['yd'], dtype=np.float64)      # list of (o,) rows -> (N,o)
            self._op = BatchedMLP(self.arch, xd, yd.reshape(xd.shape[0], -1), device=self._device,
                                  dtype=self._dtype)
            if self.kernels == "float64":
                self._op.use_exact_float64()
            if key[2] is not None:
                self._op.set_grad_data(key[2])
            self._op_key = key
        return self._op

    @staticmethod
    def _check_ltype(lpinfo):
        if lpinfo['ltype'] != 'classical':
            print('Likelihood type is not recognized. Exiting.')
            sys.exit()

    def logpost_batch(self, W, lpinfo=None):
        """Log-posterior of every row of W `(C,p)`: numpy float64 `(C,)` (with lparams['priorsigma'] set: the Gaussian weight
        prior included)."""
        lpinfo = self.lpinfo if lpinfo is None else lpinfo
        self._check_ltype(lpinfo)
        op = self._operator(lpinfo)
        if lpinfo.get('gd') is not None:
            return self._logpost_grad_data(op, np.atleast_2d(W), lpinfo, False)[0]
        sse = op.sse(np.atleast_2d(W)).cpu().numpy()
        lp = -neg_log_post_from_sse(sse, len(lpinfo['yd']), lpinfo['lparams']['sigma'])
        ps = lpinfo['lparams'].get('priorsigma')
        return lp if ps is None else lp + log_prior(W, ps)

    def logpostgrad_batch(self, W, lpinfo=None):
        """Gradient of the log-posterior for every row of W: numpy float64 `(C,p)`."""
        lpinfo = self.lpinfo if lpinfo is None else lpinfo
        self._check_ltype(lpinfo)
        op = self._operator(lpinfo)
        if lpinfo.get('gd') is not None:
            return self._logpost_grad_data(op, np.atleast_2d(W), lpinfo, True)[1]
        _, g = op.sse_grad(np.atleast_2d(W))
        sig = np.float64(lpinfo['lparams']['sigma'])
        glp = -(0.5 * g.double().cpu().numpy() / sig ** 2)
        ps = lpinfo['lparams'].get('priorsigma')
        return glp if ps is None else glp + grad_log_prior(W, ps)

    @staticmethod
    def _logpost_grad_data(op, W, lpinfo, want_grad):
        """(log-posterior (C,), its gradient (C, p) or None) with gradient observations, one `sobolev` call:
        -0.5 sse / sigma^2 - 0.5 gsse / sigma_g^2 - N o (log sigma + log(2 pi) / 2) - N o d (log sigma_g + log(2 pi) / 2),
        plus the Gaussian weight prior when lparams['priorsigma'] is set."""
        sig, sg = np.float64(lpinfo['lparams']['sigma']), np.float64(lpinfo['lparams']['sigma_g'])
        d, o = op.arch.dims[0], op.arch.dims[-1]
        cv, cg = -0.5 / sig ** 2, -0.5 / sg ** 2
        sse, gsse, g = op.sobolev(W, cv, cg, want_grad=want_grad)
        half = 0.5 * np.log(2 * np.float64(np.pi))
        lp = cv * sse.cpu().numpy() + cg * gsse.cpu().numpy() - op.N * o * (np.log(sig) + half) - op.N * o * d * (np.log(sg) + half)
        glp = g.cpu().numpy() if want_grad else None
        ps = lpinfo['lparams'].get('priorsigma')
        if ps is not None:
            lp = lp + log_prior(W, ps)
            glp = glp + grad_log_prior(W, ps) if want_grad else None
        return lp, glp

    def logpost(self, modelpars, lpinfo):
        """float: log-posterior of one flat weight vector (reference signature)."""
        return float(self.logpost_batch(np.asarray(modelpars).reshape(1, -1), lpinfo)[0])

    def logpostgrad(self, modelpars, lpinfo):
        """np.ndarray `(p,)`: gradient of the log-posterior (reference signature)."""
        return self.logpostgrad_batch(np.asarray(modelpars).reshape(1, -1), lpinfo)[0]

    # -- fit -------------------------------------------------------------------------------
    def fit(self, xtrn, ytrn, zflag=True, datanoise=0.05, nmcmc=6000, param_ini=None, sampler='amcmc',
            sampler_params=None, *, nchains=1, seeds=None, engine='host', gather='all', gather_chain=None, bfgs_jac=None,
            diagnostics=False, diag_nburn=None, gtrn=None, gradnoise=None, priorsigma=None, hyperprior=None,
            noiseprior=None):
        """Run MCMC over the flat weight vector.

        Args (reference): xtrn `(N,d)`, ytrn `(N,o)`, zflag (BFGS pre-fit of a random start),
            datanoise (likelihood sigma), nmcmc, param_ini `(p,)` [or `(C,p)`], sampler
            ('amcmc' | 'hmc' | 'mala'; build-only, engine='device': 'sgld' | 'sghmc' | 'ess' | 'nuts'), sampler_params (dict
            splatted into the sampler).
        Build-only: nchains (C independent chains in lock-step), seeds (C ints; chain c then
            equals a reference run preceded by np.random.seed(seeds[c])).  With nchains=1 and
            seeds=None the global numpy RNG is used, exactly like the reference.
            sampler_params of 'hmc' / 'mala' may hold adapt=K (both engines): the first K <= nmcmc steps are a warm-up that
            tunes a per-chain step size from `epsilon` by dual averaging (target_accept, default 0.8 / 0.574) and, unless
            adapt_mass=False, a per-chain diagonal mass matrix (`quinn_amd.mcmc.adapt`); `mcmc_results` then also holds
            'epsilon', 'mass_scale' and 'nwarm', and the warm-up rows stay in the chain (discard them with nburn >= K).
            engine='device' (samplers 'amcmc', 'hmc' and 'mala'): states, proposal factors and history stay on the
            GPU, no host synchronisation per step (`quinn_amd.mcmc.device_amcmc`); same target and
            adaptation schedule, chains equal the host engine in distribution, not bit for bit.  The device AMCMC keeps at most
            `max_rows` (sampler_params; default 4096) distinct states per chain: on longer runs older states are compressed
            into max_rows / 4 pseudo-states with the same multiplicity total, the same mean and the scatter's dominant
            max_rows / 8 directions, so the adapted proposal covariance is then a low-rank APPROXIMATION of the reference's
            full empirical covariance (exact while rank <= max_rows / 8; `DeviceAMCMC._compress_history`).
            gather (multi-rank runs; chains are block-partitioned over the ranks): 'all' -- every rank ends with all
            chains (one all_gather of the result arrays, from the device buffers in bounded pieces); 'root' -- rank 0
            does, the other ranks keep their own shard; 'none' -- no communication at all.  A gather whose result
            exceeds `quinn_amd.parallel.DEFAULT_MAX_GATHER_BYTES` raises MemoryError before any traffic.
            gather_chain: the same choice for the `chain` array alone (None: as `gather`), e.g. gather='all',
            gather_chain='none' returns MAP / acceptance / log-posterior traces of every chain everywhere and leaves the
            states sharded (at cfg2 they are 43.6 GB per rank).
            bfgs_jac: None -- the `zflag` BFGS pre-fit lets scipy difference the log-posterior, exactly as the reference
            does (nn_mcmc.py:125-127; p + 1 log-posterior evaluations per gradient); 'device' -- the gradient kernel is
            passed as the analytic jacobian (one evaluation per gradient; a different start point than the reference's).
            diagnostics: True -- after the run, split-R-hat / batch-means ESS / pooled moments of the parameters and of the
            log-posterior trace over all chains (`quinn_amd.mcmc.diagnostics`), stored as `self.diagnostics = {'params': ...,
            'logpost': ...}`.  engine='device': one device pass over the engine's own chain tensor before anything is gathered,
            so it works with gather_chain='none'; host engines: the numpy chain is uploaded in bounded pieces.  Multi-rank:
            each rank reduces its own chains, the small per-chain statistics follow `gather`.  diag_nburn: rows discarded
            first (None: nmcmc // 2).  False (default): nothing is computed and `self.diagnostics` is None.
            'rank' -- what True does, and the rank-normalised figures of `quinn_amd.mcmc.rankdiag.rank_stats` (rhat_bulk,
            rhat_tail, rhat_rank, ess_bulk, ess_tail, ess_mean, mcse_mean; their plan under rank_n_draws, rank_nh, rank_stride,
            rank_t0) merged into both dicts, from the same tensors (so also with gather_chain='none').  Ranking pools all
            chains: with more than one rank and chains the calling rank does not hold it is a ValueError.
            sampler_params of 'hmc' / 'mala' with engine='device' may hold ladder=R (or a decreasing sequence of inverse
            temperatures starting at 1), beta_min (default 0.01) and swap_every (default 1): replica exchange
            (`quinn_amd.mcmc.tempering`).  The nchains chains are nchains / R ladders, chain c is rung c % R and samples
            pi^beta_r; `mcmc_results` then also holds 'beta', 'swap_rate' and 'replica', and predict_ens / score with
            chain='all', diagnostics=True and `diagnose` use the cold chains (beta == 1) only.  nchains (and every rank's
            shard) must be a multiple of R; use_graph=True is refused.
            sampler='sgld' | 'sghmc' (engine='device' only; `quinn_amd.mcmc.device_sgmcmc`): stochastic-gradient Langevin /
            Hamiltonian dynamics, every chain on its own minibatch drawn on the device.  sampler_params: eta (step size),
            alpha ('sghmc' only: friction in (0, 1], default 0.1), batch (rows per chain and step, with replacement; None: all
            rows), thin (every thin-th state is stored: nmcmc stored rows are nmcmc * thin inner steps), schedule
            ('constant' | 'cyclic'), cycles and explore_frac (cyclic: cosine cycles over the run; the head of each cycle runs
            without noise), temperature (default 1), use_graph, groups.  There is no accept test ('accrate' and 'alphas' are 1)
            and 'logpost' is the minibatch estimate of each stored state's log-posterior.
            sampler='ess' (engine='device' only; `quinn_amd.mcmc.device_ess`): elliptical slice sampling.  Needs priorsigma
            (the ellipse is drawn from the prior); no step size, no warm-up, forward calls only.  sampler_params: max_shrink
            (proposals per step before the step is truncated and the chain stays; default 32), block (iterations enqueued
            between two looks at the chains' step counters; default 32), groups.  The chains advance asynchronously on the
            device; `mcmc_results` also holds 'nev' `(C, nmcmc + 1)` (forward evaluations per step), 'ntrunc' and 'nevals'
            `(C,)`; 'accrate' is 1 - ntrunc / nmcmc and 'alphas' is 1.
            sampler='nuts' (engine='device' only; `quinn_amd.mcmc.device_nuts`): the No-U-Turn sampler, multinomial, in whitened
            momenta.  No trajectory length: a step doubles its trajectory until it turns back on itself.  sampler_params:
            epsilon (the step size, a scalar or one per chain), mass_scale (None, or `(nchains, p)`: e.g. 'mass_scale' of an
            'hmc' fit with adapt=K, with its 'epsilon'), max_depth (doublings per step, 1 .. 12; default 10), adapt (warm-up
            steps of step-size dual averaging), adapt_mass (default False; True: the warm-up also finds a per-chain diagonal
            mass over the windows of `warmup_schedule(adapt)`, `quinn_amd.mcmc.nuts_adapt`, and `mcmc_results` holds
            'mass_scale' `(C, p)`; needs adapt > 0), target_accept (default 0.8), block, groups.  The chains advance asynchronously on the device; `mcmc_results` also holds 'depth' and 'nleap'
            `(C, nmcmc + 1)` (doublings and leapfrogs per step), 'ndiv', 'ntreedepth', 'ngrad' and 'epsilon' `(C,)` and 'nwarm';
            'alphas' is the acceptance statistic of each step and 'accrate' its mean.  float64 operators only; no ladder, no
            graph capture.
            gtrn `(N, d)` | `(N, o, d)` with gradnoise (sigma_g): observed input gradients as a second Gaussian likelihood
            term, log-posterior -0.5 sse / sigma^2 - 0.5 gsse / sigma_g^2 - N o (log sigma + log(2 pi) / 2)
            - N o d (log sigma_g + log(2 pi) / 2) with gsse = sum (dM/dx - gtrn)^2; engine='host' only (the device engines'
            accept kernels take a bare SSE).
            priorsigma: None (default) -- no prior, the reference's target; s > 0 -- the isotropic Gaussian weight prior
            N(0, s^2 I) (`quinn_amd.mcmc.prior`), stored as lpinfo['lparams']['priorsigma'].  `logpost` / `logpostgrad` and
            their batched forms then include log N(w; 0, s^2 I) (normaliser included) and -w / s^2, so the host samplers and
            the `zflag` BFGS pre-fit (which becomes the MAP with the prior) need no change; engine='device' hands s to the
            engine, which folds the prior into every SSE / gradient on the GPU (qn_prior_fold): 'logpost', 'maxpost' and
            the MAP of every engine are those of the posterior with the prior, on every rung of a ladder (whose beta
            tempers likelihood and prior alike: a hot rung's prior has variance s^2 / beta).  The SG samplers' prior is
            exact, only their likelihood is a minibatch estimate.  One scalar s: no per-layer or ARD scales, no hyper-prior.
            Anything but None or a finite s > 0 raises ValueError before any launch.

            hyperprior: None (default; exactly the launches made without the argument) or dict(a0=, b0=, groups='layer' |
            'tensor' | 'all', every=1, tau0=None) -- the hierarchical prior of `quinn_amd.mcmc.hyper`: a zero-mean Gaussian
            per weight group ('layer': each Linear's weight and bias; 'tensor': every parameter tensor; 'all': one group; at
            most 32) whose precision tau_g ~ Gamma(shape a0, rate b0) is Gibbs-sampled on the device after every `every`-th
            step, per chain.  Initial precisions: tau0 (a scalar or one per group), else 1 / priorsigma^2, else a0 / b0.
            every=0 never draws: fixed per-group scales from tau0 (required then).  sampler='hmc' | 'mala' with
            engine='device' only (with adapt, groups, gather_chain, diagnostics, predict_ens, score and rank sharding); not
            with a ladder, use_graph=True or a residual network: ValueError.  'logpost' / 'maxpost' and the MAP bookkeeping are
            then those of the JOINT density of (w, tau) (`hyper.log_joint`), a function of the chain's whole state, so the
            R-hat of its trace means something; a joint mode in tau is of limited use -- predict with `predict_ens` /
            `score`, not from the MAP.  mcmc_results gains 'tau' [C, nrounds + 1, G] (the precisions after every round; column
            0 the initial ones) and 'prior_groups' [(name, lo, hi)]; the settings are stored in lpinfo['lparams']['hyperprior'].

            noiseprior (keyword only): None (default; exactly the launches made without the argument) or dict(a0=, b0=,
            every=1, sigma_init=None) -- the noise prior of `quinn_amd.mcmc.noise`: one noise variance s2 per chain with
            1 / s2 ~ Gamma(shape a0, rate b0), Gibbs-sampled on the device after every `every`-th step, started at
            sigma_init, else at datanoise (which stays the kernels' nominal unit and no longer matters otherwise).  The weight
            prior is not scaled by s2.  every=0 never draws: a fixed level sigma_init (a0, b0 may be omitted).
            sampler='hmc' | 'mala' with engine='device' only (with adapt, groups, priorsigma, hyperprior, gather_chain,
            diagnostics and rank sharding); not with a ladder, use_graph=True, a residual network or float32 kernels:
            ValueError.  'logpost' / 'maxpost' are then the JOINT density of (w, s2[, tau]) (`noise.log_joint`).  mcmc_results
            gains 'sigma' [C, nrounds + 1] (column 0: the initial level); stored row t >= 1 pairs with sigma[:, t // every]
            (every=0 and row 0: column 0), `noise_samples` returns the levels of the rows `predict_ens` picks, and `score`
            with noise=None scores every member at its own level.  The settings are stored in
            lpinfo['lparams']['noiseprior'].
        """
        self.diagnostics = None
        priorsigma = check_priorsigma(priorsigma)
        if seeds is not None:
            seeds = list(seeds)
        if engine == 'device':                   # every refusal that host values decide, before any device is touched
            if sampler not in DEVICE_ENGINES:
                raise ValueError("engine='device' is implemented for sampler='amcmc', 'hmc', 'mala', 'sgld', 'sghmc', 'ess' and "
                                 "'nuts'")
            # (the chains of the run: the rows of a 2-D param_ini, else one per seed)
            ctot = np.shape(param_ini)[0] if np.ndim(param_ini) > 1 else nchains if seeds is None else len(seeds)
            cfg = DEVICE_ENGINES[sampler].check_params(self.arch, self._dtype, nmcmc, priorsigma, nchains=ctot,
                                                       hyperprior=hyperprior, noiseprior=noiseprior, **(sampler_params or {}))
        else:
            if sampler in DEVICE_ONLY:
                raise ValueError(f"sampler={sampler!r} runs on the GPU only: pass engine='device' (there is no host engine for it)")
            for name, val in (('hyperprior', hyperprior), ('noiseprior', noiseprior)):
                if val is not None:
                    raise ValueError(priors_refusal(name, sampler, engine))
            cfg = {'priorsigma': priorsigma}
        diag_nburn = nmcmc // 2 if diag_nburn is None else int(diag_nburn)
        ntrn_, outdim = ytrn.shape
        assert xtrn.shape[0] == ntrn_
        self.lpinfo = {'model': None, 'xd': xtrn, 'yd': [y for y in ytrn], 'ltype': 'classical',
                       'lparams': {'sigma': datanoise}}
        for k in ('priorsigma', 'hyperprior', 'noiseprior'):
            if cfg.get(k) is not None:
                self.lpinfo['lparams'][k] = cfg[k]
        if gtrn is not None:
            if engine == 'device':
                raise NotImplementedError("gradient observations (gtrn) need engine='host': the device samplers' accept "
                                          "kernels take a bare sum of squared errors")
            if gradnoise is None or not float(gradnoise) > 0.0:
                raise ValueError("gtrn needs gradnoise > 0, the noise level of the gradient observations")
            self.lpinfo['gd'] = check_gradloss_args(self.arch, self._dtype, xtrn, gtrn, 0.0)
            self.lpinfo['lparams']['sigma_g'] = float(gradnoise)
        elif gradnoise is not None:
            raise ValueError("gradnoise goes with gtrn")
        if seeds is not None:
            nchains = len(seeds)
            rngs = [np.random.RandomState(s) for s in seeds]
        elif nchains > 1:
            raise ValueError("nchains > 1 needs seeds=[...] (one per chain)")
        else:
            rngs = None

        if param_ini is None:
            draw = (lambda r: r.rand(self.pdim)) if rngs else (lambda r: np.random.rand(self.pdim))
            inis = [draw(r) for r in (rngs or [None])]
            if zflag:
                # BFGS pre-fit of the random start (nn_mcmc.py:125-127); finite differences by default, like the reference
                if bfgs_jac not in (None, 'device'):
                    raise ValueError("bfgs_jac is None (scipy differences the log-posterior) or 'device'")
                jac = (lambda x, fcn, lpinfo: -self.logpostgrad(x, lpinfo)) if bfgs_jac == 'device' else None
                inis = [minimize((lambda x, fcn, lpinfo: -fcn(x, lpinfo)), ini, args=(self.logpost, self.lpinfo), jac=jac,
                                 method='BFGS', options={'gtol': 1e-13}).x for ini in inis]
            param_ini = np.stack(inis) if rngs else inis[0]
        param_ini = np.asarray(param_ini, dtype=np.float64)
        if rngs and param_ini.ndim == 1:
            param_ini = np.tile(param_ini, (nchains, 1))

        sampler_params = dict(sampler_params)      # None raises, as in the reference
        nadapt = int(sampler_params.get('adapt', 0) or 0)
        if nadapt > nmcmc:
            raise ValueError(f"sampler_params['adapt'] = {nadapt} warm-up steps exceed nmcmc = {nmcmc}")
        if engine == 'device':
            self._fit_device(DEVICE_ENGINES[sampler], cfg, sampler_params, nmcmc, param_ini, seeds, gather, gather_chain,
                             diagnostics, diag_nburn)
        else:
            self._fit_host(sampler, sampler_params, nmcmc, param_ini, seeds, rngs, gather, gather_chain, diagnostics, diag_nburn)

    def _fit_device(self, engine_cls, cfg, sampler_params, nmcmc, param_ini, seeds, gather, gather_chain, diagnostics, diag_nburn):
        """The run of `fit(engine='device')` after the common prologue.  cfg: what the engine's `check_params` returned."""
        ini2 = np.atleast_2d(param_ini)
        ctot = ini2.shape[0]
        rank, world = dist_info()
        lo, hi = shard_bounds(ctot) if world > 1 else (0, ctot)      # chains shard over ranks
        # replica exchange: this rank's shard of the chains, like all of them, is whole ladders (refused before any launch)
        R = None if cfg.get('ladder') is None else cfg['ladder'].size
        if R is not None:
            check_whole_ladders(R, hi - lo, lo)
        op = self._operator(self.lpinfo)
        priors = {k: cfg[k] for k in ('hyperprior', 'noiseprior') if cfg.get(k) is not None}
        # random streams are keyed by the GLOBAL chain id: results do not depend on the number of ranks
        eng = engine_cls(op, self.lpinfo['lparams']['sigma'], seed=seeds[0] if seeds else 0, chain0=lo, priorsigma=cfg['priorsigma'],
                         **engine_cls.shard_params(sampler_params, lo, hi), **priors)
        res = eng.run(nmcmc, ini2[lo:hi], verbose=self.verbose and rank == 0) if hi > lo else eng.empty_results(nmcmc)
        if diagnostics:
            # from the engine's device tensors, before they are downloaded (or not: gather_chain='none'); of a
            # replica-exchange run the cold chains only (rung 0 of every ladder: shards are whole ladders)
            dch, dlp, dtot = res['chain'], res['logpost'], ctot
            if R is not None:
                if dch is None:
                    raise ValueError("diagnostics=True needs the stored chain")
                cp = (lambda v: v.contiguous()) if isinstance(dch, torch.Tensor) else np.ascontiguousarray
                dch, dlp, dtot = cp(dch[::R]), cp(dlp[::R]), ctot // R        # (a copy of 1 / R of the chain)
            self.diagnostics = self._fit_diagnostics(dch, dlp, diag_nburn, dtot, gather, rank=diagnostics == 'rank')
        # the single collective, at the end, straight from the device tensors (world == 1: a device->host copy)
        self.mcmc_results = gather_results(res, ctot, gather, gather_chain)
        if np.ndim(param_ini) == 1:
            self.mcmc_results = {k: (v[0] if isinstance(v, np.ndarray) else v) for k, v in self.mcmc_results.items()}
        if cfg.get('prior_groups') is not None:
            self.mcmc_results['prior_groups'] = cfg['prior_groups']
        self.samples, self.cmode = self.mcmc_results['chain'], self.mcmc_results['mapparams']

    def _fit_host(self, sampler, sampler_params, nmcmc, param_ini, seeds, rngs, gather, gather_chain, diagnostics, diag_nburn):
        """The run of `fit(engine='host')` after the common prologue."""
        if sampler not in HOST_SAMPLERS:
            raise ValueError(f"sampler {sampler!r} is not one of 'amcmc', 'hmc', 'mala'")
        sampler_cls, with_grad = HOST_SAMPLERS[sampler]
        mymcmc = sampler_cls(**sampler_params)
        mymcmc.setLogPostBatch(self.logpost_batch, self.logpostgrad_batch if with_grad else None, lpinfo=self.lpinfo)
        sharded = rngs is not None and dist_info()[1] > 1
        if sharded:
            # chains shard over ranks; one all_gather of the result arrays at the end
            self.mcmc_results = run_chains_sharded(lambda: mymcmc, nmcmc, param_ini, seeds, verbose=False, gather=gather, gather_chain=gather_chain)
        else:
            self.mcmc_results = mymcmc.run(nmcmc=nmcmc, param_ini=param_ini, rngs=rngs, verbose=self.verbose)
        self.samples, self.cmode = self.mcmc_results['chain'], self.mcmc_results['mapparams']
        if diagnostics:
            ch, lp = np.asarray(self.mcmc_results['chain']), np.asarray(self.mcmc_results['logpost'])
            if ch.ndim == 2:
                ch, lp = ch[None], lp[None]
            ctot = len(seeds) if sharded else ch.shape[0]
            if sharded and ch.shape[0] == ctot:      # gathered chains: every rank reduces its own shard only
                lo, hi = shard_bounds(ctot)
                ch, lp = ch[lo:hi], lp[lo:hi]
            self.diagnostics = self._fit_diagnostics(ch, lp, diag_nburn, ctot if sharded else None, gather,
                                                     rank=diagnostics == 'rank')

    def _fit_diagnostics(self, chain, lps, nburn, ctot, gather, rank=False):
        """{'params', 'logpost'}: diagnostics of this rank's chains `[C, T, p]` and log-posterior traces `[C, T]`
        (device tensors or numpy), the per-chain statistics gathered over the ranks as `gather` says.  rank: the figures of
        `rankdiag.rank_stats` are merged in (they pool the chains, so every chain must be here)."""
        if chain is None:
            raise ValueError("diagnostics=True needs the stored chain")
        dev = self._device
        if rank and ctot is not None and dist_info()[1] > 1 and chain.shape[0] != ctot:
            raise ValueError(f"diagnostics='rank' ranks the pooled draws of all {ctot} chains; this rank holds {chain.shape[0]} "
                             "(rank diagnostics across ranks are not covered)")
        out = {'params': diag.diagnose_chains(chain, nburn, n_total=ctot, gather=gather, device=dev),
               'logpost': diag.diagnose_chains(lps[..., None], nburn, n_total=ctot, gather=gather, device=dev)}
        if rank:
            for key, ch in (('params', chain), ('logpost', lps[..., None])):
                if out[key] is not None:
                    out[key].update(_rank_keys(rankdiag.rank_stats(ch, nburn, device=dev)))
        return out

    def diagnose(self, x=None, nburn=1000, nens=100, rank=False):
        """Diagnostics of `self.samples` (`[C, T, p]`; one 2-D chain counts as C = 1) after `nburn` rows: {'params': ...}
        as `fit(diagnostics=True)` computes it.  With x `(N, d)` also FUNCTION-SPACE diagnostics under 'pred': `nens` draws
        per chain thinned by the reference's rule (rows nburn + j * int((T - nburn) / nens)), all C * nens predictions from
        one batched forward, and the same statistics over the `[C, nens, N * o]` stack; rhat / ess / mean / var there
        have shape `(N, o)`.  Predictions, unlike weights, do not change when hidden units are permuted.
        rank=True merges the rank-normalised figures (`fit(diagnostics='rank')` names them) into 'params' and 'pred'; the
        prediction figures have shape `(N, o)`."""
        samples = np.asarray(self.samples)
        if samples.ndim == 2:
            samples = samples[None]
        cold = self._cold_chains()
        if cold is not None:
            samples = samples[cold]
        out = {'params': diag.diagnose_chains(samples, nburn, device=self._device)}
        if rank:
            out['params'].update(_rank_keys(rankdiag.rank_stats(samples, nburn, device=self._device)))
        if x is not None:
            C, T, p = samples.shape
            rows = diag.thinned_rows(T, nens, nburn)
            y = self._predict_batch_dev(samples[:, rows, :].reshape(C * nens, p), x)        # (C * nens, N, o)
            N, o = y.shape[1], y.shape[2]
            if y.dtype not in (torch.float32, torch.float64):
                y = y.double()
            pred = diag.diagnose_chains(y.contiguous().view(C, nens, N * o), 0)
            for k in ('rhat', 'ess', 'mean', 'var'):
                pred[k] = pred[k].reshape(N, o)
            if rank:
                rk = _rank_keys(rankdiag.rank_stats(y.contiguous().view(C, nens, N * o), 0))
                pred.update((k, v.reshape(N, o) if isinstance(v, np.ndarray) else v) for k, v in rk.items())
            out['pred'] = pred
        return out

    # -- prediction --------------------------------------------------------------------------
    def get_best_model(self, param):
        """A copy of the module carrying the given flat weight vector (nn_mcmc.py:142-154)."""
        import torch
        mod = copy.deepcopy(self.nnmodel)
        s = 0
        with torch.no_grad():
            for p in mod.parameters():
                n = p.numel()
                p.copy_(torch.as_tensor(np.asarray(param[s:s + n])).view(p.shape).to(p.dtype))
                s += n
        return mod

    def predict_sample(self, x, param):
        """`(N,o)` prediction with one flat weight vector (nn_mcmc.py:168-178)."""
        return self._predict_batch(np.asarray(param).reshape(1, -1), x)[0]

    def predict_MAP(self, x, chain=None):
        """Prediction with the MAP weights: chain None -- the first chain's (the only one of a reference-style run);
        'best' -- those of the chain with the largest `maxpost`; an int -- that chain's."""
        if np.ndim(self.cmode) == 1:
            cm = self.cmode
        elif chain == 'best':
            cm = self.cmode[int(np.argmax(self.mcmc_results['maxpost']))]
        else:
            cm = self.cmode[0 if chain is None else chain]
        return self.predict_sample(x, cm)

    def _cold_chains(self):
        """Indices of the cold chains (beta == 1) of a replica-exchange fit whose results this rank holds for every stored
        chain; None for any other fit."""
        beta = getattr(self, 'mcmc_results', {}).get('beta')
        if beta is None or np.ndim(beta) != 1 or np.ndim(self.samples) != 3 or len(beta) != self.samples.shape[0]:
            return None
        return np.flatnonzero(np.asarray(beta) == 1.0)

    def _ens_picks(self, nens=10, nburn=1000, chain=0):
        """[(chain index into `self.samples` (None: one 2-D chain), rows)]: the stored rows of the predictive ensemble."""
        nens = 10 if nens is None else nens
        if isinstance(chain, str):
            if chain != 'all':
                raise ValueError("chain is an int or 'all'")
            shape = self.samples.shape if self.samples.ndim == 3 else (1,) + self.samples.shape
            cold = self._cold_chains()
            ids = np.arange(shape[0]) if cold is None else cold
            picks = diag.pooled_rows(len(ids), shape[1], nens, nburn)
            return [(int(ids[c]) if self.samples.ndim == 3 else None, rows) for c, rows in picks]
        T = self.samples.shape[0] if self.samples.ndim == 2 else self.samples.shape[1]
        nevery = int((T - nburn) / nens)
        return [(None if self.samples.ndim == 2 else chain, [nburn + j * nevery for j in range(nens)])]

    def _ens_weights(self, nens=10, nburn=1000, chain=0):
        picks = self._ens_picks(nens, nburn, chain)
        if isinstance(chain, str):
            return np.concatenate([(self.samples if c is None else self.samples[c])[rows, :] for c, rows in picks])
        c, rows = picks[0]
        return (self.samples if c is None else self.samples[c])[rows, :]

    def noise_samples(self, nens=10, nburn=1000, chain=0):
        """`(M,)`: the noise level of every member of the ensemble `predict_ens(x, nens, nburn, chain)` evaluates, after a fit
        with `noiseprior`: stored row t >= 1 of a chain was drawn at sigma[c, t // every] (every = 0 and row 0: column 0)."""
        nprior = getattr(self, 'lpinfo', {}).get('lparams', {}).get('noiseprior')
        if nprior is None or 'sigma' not in getattr(self, 'mcmc_results', {}):
            raise ValueError("noise_samples needs a fit with noiseprior=")
        sigma = np.atleast_2d(self.mcmc_results['sigma'])
        every = nprior['every']
        return np.concatenate([sigma[0 if c is None else c, (np.asarray(rows) // every) if every else np.zeros(len(rows), dtype=int)]
                               for c, rows in self._ens_picks(nens, nburn, chain)])

    def _score_member_noise(self, noise, nsam, **ens_args):
        """After a fit with `noiseprior`, noise=None scores every member at its own sampled level."""
        if noise is None and getattr(self, 'lpinfo', None) and self.lpinfo['lparams'].get('noiseprior') is not None:
            return self.noise_samples(nsam, **ens_args)
        return None

    def stack(self, x, y, nsam=1000, nburn=1000, loo=True, noise=None, tol=scoring.DEFAULT_TOL, max_iter=scoring.DEFAULT_MAX_ITER,
              max_bytes=256 << 20):
        """Stacking weights of the chains (Yao, Vehtari & Gelman 2022): chains that did not mix are not pooled with equal
        weights but with the weights on the simplex that maximise the log predictive density of the weighted mixture on
        (x, y).  The groups are the chains of `chain='all'` (the cold chains after a ladder fit), chain c with its nsam // C +
        (c < nsam % C) thinned draws.  loo=True (x, y the training data): a chain's density of an entry is its PSIS-LOO
        density (`qn_psis_loo` per chain; at least 2 draws per chain); loo=False (held-out data): its plain predictive density
        (`qn_group_lpd`).  x is walked in the row chunks of `score`, the `[C, N * o]` matrix stays on the device, and
        `qn_stack_weights` iterates EM to a certified gap of `tol` nats.  A sampled noise level goes through V as in `score`.
        Returns and stores as `self.stacking`: `weights` `(C,)`, `member_weights` `(M,)` (for `score(member_weights=...)`
        and `predict_mom_stacked`, with the same nsam, nburn and chain='all'), `elpd_stack` and `elpd_equal` (the objective at
        the weights and at 1 / C), `gap`, `iters`, `n_dropped`, `n_nonfinite`, `khat_bad_share` `(C,)` (loo only: the share
        of entries whose khat is above the threshold, per chain), `offsets`, `nsam`, `ens_args`."""
        if self.samples is None or np.ndim(self.samples) != 3:
            raise ValueError("stack needs the stored chains of a multi-chain fit")
        maxpost = np.atleast_1d(self.mcmc_results.get('maxpost', np.empty(self.samples.shape[0])))      # gathered from every rank
        if len(maxpost) != self.samples.shape[0]:
            raise ValueError("this rank does not hold every chain (gather_chain='none' across ranks): stack needs them all")
        ens_args = dict(nburn=nburn, chain='all')
        picks = self._ens_picks(nsam, nburn, 'all')
        offsets = np.concatenate([[0], np.cumsum([len(rows) for _, rows in picks])])
        member = self._score_member_noise(noise, nsam, **ens_args)
        sigma = self._score_noise(noise) if member is None else 0.0
        res = self._stack_groups(x, y, self._ens_weights(nsam, **ens_args), offsets, member, sigma, loo, tol, max_iter, max_bytes)
        res.update(nsam=nsam, ens_args=ens_args)
        return res

    def _predict_ens_dev(self, x, nens=10, nburn=1000, chain=0):
        return self._predict_batch_dev(self._ens_weights(nens, nburn, chain), x)

    def predict_ens(self, x, nens=10, nburn=1000, chain=0):
        """`(M,N,o)`: predictions with M thinned post-burn-in samples, rows
        nburn + j*int((len-nburn)/nens) of the chain (nn_mcmc.py:194-199) -- one batched
        forward instead of M sequential ones.  `chain` picks the chain of a multi-chain fit; chain='all' pools the
        chains: chain c contributes nens // C + (c < nens % C) draws, thinned by the same rule with that count, ordered
        chain-major, still one batched forward.  After a replica-exchange fit chain='all' pools the cold chains (beta == 1)
        only; an int indexes all chains as before."""
        return self._predict_ens_dev(x, nens, nburn, chain).double().cpu().numpy()
