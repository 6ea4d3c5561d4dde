"""Hamiltonian Monte Carlo with states, momenta and history resident on the GPU (throughput engine).

Same leapfrog scheme and accept rule as the reference (quinn/mcmc/hmc.py:43-66, mcmc.py:65-85): momentum ~ N(0, I),
half kick, L drifts with L-1 inner kicks, half kick.  One step is a static sequence of launches through the C ABI and
nothing else -- no torch op, no host synchronisation:

    qn_hmc_begin   momenta (in-kernel Philox keyed by the GLOBAL chain id), K_cur partials, half kick with the cached
                   gradient of the current state, first drift
    L x [ qn_mlp_sse_fwdbwd at q  ->  qn_hmc_leap (kick + drift; last: half kick + K_prop partials) ]
    qn_hmc_accept  log-posterior of the proposal from the SSE of the LAST gradient call, MH test, state / gradient /
                   MAP / history rows, device step counter (double-buffered by step parity, as in the AMCMC engine)

so L gradient launches per step instead of the reference's L + 1 gradients + 1 forward (the gradient at the current
state is the accepted proposal's, the proposal's log-posterior comes with its gradient).  With `use_graph=True` pairs
of steps (parity 0, 1) are captured once in a HIP graph and replayed.  Random streams are keyed by (seed, step, global
chain id): a chain's path does not depend on how the chains are split over ranks or launches (only the summation order
of its SSE does, through the row split the gradient kernel picks for the batch size).  Chains agree with the host `HMC`
in distribution, not bit for bit (Philox instead of numpy's MT19937).  Every begin / leap entry point named here and below
is an instantiation of the one kernel pair of csrc/qn_hmc_leap.hip; the accept calls are in csrc/qn_mcmc.hip.

`adapt` > 0 warm-up steps tune a per-chain step size and, with `adapt_mass`, a per-chain diagonal mass matrix on the device
(`quinn_amd.mcmc.adapt` states the contract): every step then runs qn_hmc_begin_s / qn_hmc_leap_s, which read the step
sizes [C] and the scales [C, p] from device arrays; a warm-up step is followed by one qn_hmc_adapt launch whose schedule
(window ends, counts) is static and host-known, so still nothing is read back.  Warm-up rows are stored like any other row
(discard them with `nburn`); the results gain 'epsilon' [C], 'mass_scale' [C, p] (None without mass windows) and 'nwarm'.
adapt = 0 (default) runs the fixed-step kernels exactly as before.

`ladder` (an int R or a sequence of inverse temperatures) turns the chains into C / R replica-exchange ladders
(`quinn_amd.mcmc.tempering` states the contract): chain c is rung c % R and samples pi^beta_r through qn_hmc_begin_t /
qn_hmc_leap_t / qn_hmc_accept_t, from the per-chain step size epsilon / sqrt(beta_r) (the exact scaling for a Gaussian target;
`adapt` then tunes each rung's step and mass as before), and every `swap_every`-th step, warm-up included, is followed by one
qn_pt_swap launch (order within a step: accept, adapt, swap).  The results gain 'beta' [C], 'swap_rate' [C] (accepted / tried
exchanges with the next rung; NaN for the top rung) and 'replica' [C, nrounds + 1] (the replica in each chain slot after every
round; column 0 is the global chain id).  Use the cold chains (beta == 1) for inference.  A ladder cannot be captured in a graph.
ladder = None (default) runs exactly what ran before, through the same entry points.

`priorsigma` = s puts the Gaussian weight prior N(0, s^2 I) on the target (`quinn_amd.mcmc.prior`): one qn_prior_fold launch behind
the initial and every leapfrog gradient call adds lam |q|^2 + c0 to the SSE and 2 lam q to the gradient (q: the float64 positions),
and everything above -- forces, accept test, warm-up, ladder, graph, groups -- runs on the posterior with the prior, untouched.
priorsigma = None (default) makes no such launch.

`hyperprior` = dict(a0=, b0=, groups='layer' | 'tensor' | 'all', every=1, tau0=None) replaces the one scalar by a precision per
weight group and chain with a Gamma(a0, rate b0) hyper-prior (`quinn_amd.mcmc.hyper` states the contract): the run state gains
the device arrays s['lam'] [2, C, G], s['c0'] [2, C] (double-buffered by the parity s['hpar'] of their own), s['seg'] [G + 1] and
s['taus'] [C, nrounds + 1, G]; while s['lam'] is set, qn_prior_fold_g stands where qn_prior_fold stood, and every `every`-th
step, warm-up included, is followed by one qn_hyper_gibbs launch (order within a step: accept, adapt, Gibbs round) that draws
the precisions and refreshes the cached gradient and log density of the current state.  'logpost' / 'maxpost' are then the JOINT
log density of (w, tau); the results gain 'tau' [C, nrounds + 1, G] (column 0: the initial precisions, tau0, else
1 / priorsigma^2, else a0 / b0) and the engine the attribute `prior_groups` [(name, lo, hi)].  every = 0 never draws (fixed
per-group scales from tau0).  Not with a ladder or a graph.  hyperprior = None (default) makes exactly the launches made before.

`noiseprior` = dict(a0=, b0=, every=1, sigma_init=None) samples the noise level too (`quinn_amd.mcmc.noise` states the contract):
one variance s2 per chain with 1 / s2 ~ Gamma(a0, rate b0), started at sigma_init, else at `sigma`.  The kernels keep the nominal
`sigma`; the run state gains s['kappa'], s['d0'] [2, C] (double-buffered by the parity s['npar'] of their own), s['sig']
[C, nrounds + 1] and the round counter s['nround'].  While s['kappa'] is set, ONE qn_noise_fold launch stands where qn_prior_fold /
qn_prior_fold_g stood -- it carries the weight prior too: the current lam / c0 / seg of a hyper-prior, a one-group lam from
`priorsigma`, or no group -- and every `every`-th step, warm-up included, is followed by one qn_noise_gibbs launch (order within
a step: accept, adapt, hyper round, noise round).  'logpost' / 'maxpost' are then the JOINT log density of (w, s2[, tau]); the
results gain 'sigma' [C, nrounds + 1] (column 0: the initial level).  every = 0 never draws: a fixed level sigma_init through the
same fold (a0, b0 may be omitted).  Not with a ladder, a graph, a residual network or a float32 operator.  noiseprior = None
(default) makes exactly the launches made before.

The three folds are one kernel (csrc/qn_prior.hip) behind three entry points, and the engine says the choice once: `_fold` picks
qn_noise_fold, else qn_prior_fold_g, else qn_prior_fold, else nothing from what the run state holds, for the initial state and for
every leapfrog gradient alike.  Likewise `_gibbs_step` is the one order after a step -- accept, adapt, exchange round, hyper
round, noise round, a round after every s['severy']-th / s['hevery']-th / s['nevery']-th step (absent or 0: never) -- for the
warm-up and for every run that has a round; a run without rounds takes plain `_step`s, and pairs of those are captured in a graph.
"""
import numpy as np
import torch

from .. import _lib
from .adapt import TARGET_ACCEPT, check_adapt_args, warmup_plan
from .hyper import check_hyperprior, check_segments, fold_constants_g, group_segments, initial_tau
from .noise import check_noiseprior, fold_constants_n
from .tempering import check_temper_args, check_whole_ladders
from .device_engine import DeviceEngine


def _ptr(t):
    return None if t is None else t.data_ptr()


class DeviceHMC(DeviceEngine):
    _kind = 'hmc'

    @classmethod
    def check_params(cls, arch, dtype, nmcmc, priorsigma, nchains=None, chain0=0, hyperprior=None, noiseprior=None, L=3,
                     use_graph=False, adapt=0, target_accept=None, ladder=None, beta_min=0.01, swap_every=1, **rest):
        if int(L) < 1:
            raise ValueError("HMC needs L >= 1 leapfrog steps")
        cfg = super().check_params(arch, dtype, nmcmc, priorsigma)
        # warm-up: `adapt` steps of dual averaging from `epsilon` towards `target_accept` (default 0.8; MALA 0.574)
        cfg['target_accept'] = TARGET_ACCEPT[cls._kind] if target_accept is None else float(target_accept)
        cfg['adapt'] = check_adapt_args(adapt, cfg['target_accept'])
        # replica exchange: the inverse temperatures of one ladder (None: no tempering); all chains are whole ladders
        cfg['ladder'] = None if ladder is None else check_temper_args(ladder, beta_min, swap_every, C=nchains, chain0=chain0,
                                                                      use_graph=use_graph)
        # hierarchical prior and noise prior: the settings (None: the scalar prior or none; the hand-set noise level)
        cfg['hyperprior'], cfg['noiseprior'] = check_hyperprior(hyperprior), check_noiseprior(noiseprior)
        for name, own, what in (('hyperprior', 'precisions', 'weight groups are defined'),
                                ('noiseprior', 'noise level', 'the noise level is sampled')):
            if cfg[name] is None:
                continue
            if cfg['ladder'] is not None:
                raise ValueError(f"{name} does not run with a ladder (a tempered rung would need its own {own})")
            if use_graph:
                raise ValueError(f"{name} does not run with use_graph=True (the round counter changes from launch to launch)")
            if type(arch).__name__ != 'MLPArch':
                raise ValueError(f"{name}: {what} for plain MLPs, not for a residual network (RNet)")
        if cfg['noiseprior'] is not None and dtype != 'float64':
            raise ValueError("noiseprior needs a float64 operator (the fold's rescaling of a float32 gradient would round it "
                             "a second time)")
        cfg['seg'] = cfg['prior_groups'] = None
        if cfg['hyperprior'] is not None:                  # the weight groups, known before any launch
            seg, names = group_segments(arch, cfg['hyperprior']['groups'])
            cfg['seg'] = check_segments(seg, arch.nparams)
            initial_tau(cfg['hyperprior'], len(names), cfg['priorsigma'])      # (a tau0 of the wrong length is refused here)
            cfg['prior_groups'] = [(n, int(lo), int(hi)) for n, lo, hi in zip(names, seg[:-1], seg[1:])]
        return cfg

    def __init__(self, op, sigma, epsilon=0.05, L=3, seed=0, chain0=0, use_graph=False, groups=None, adapt=0,
                 target_accept=None, adapt_mass=True, ladder=None, beta_min=0.01, swap_every=1, priorsigma=None, hyperprior=None,
                 noiseprior=None):
        # groups: default 1.  Unlike the AMCMC engine's forward (two workgroups per CU, a lone one runs 1.8 x faster) the gradient
        # kernel puts ONE workgroup on a CU, so a group's launch cannot spread into the CUs the other group's small kernels leave
        # idle -- measured at cfg2: 1418 -> 1427 steps/s (HMC, L = 3), 4094 -> 4100 (MALA)
        cfg = self.check_params(op.arch, op.dtype, None, priorsigma, chain0=chain0, hyperprior=hyperprior, noiseprior=noiseprior,
                                L=L, use_graph=use_graph, adapt=adapt, target_accept=target_accept, ladder=ladder,
                                beta_min=beta_min, swap_every=swap_every)
        self.epsilon, self.L = float(epsilon), int(L)
        super().__init__(op, sigma, seed, chain0, use_graph, groups, priorsigma)
        self.target_accept, self.adapt, self.adapt_mass = cfg['target_accept'], cfg['adapt'], bool(adapt_mass)
        self.beta_min, self.swap_every = float(beta_min), swap_every           # (the steps between two exchange rounds)
        self._ladder, self._hyper, self._noise = cfg['ladder'], cfg['hyperprior'], cfg['noiseprior']
        self._seg, self.prior_groups = cfg['seg'], cfg['prior_groups']

    def _begin(self, s, st):
        """Enqueue the begin call of a step.  The entry point follows from what the state holds: s['beta'] (a ladder) -> _t,
        else s['eps'] (a device step size: warm-up) -> _s, else the fixed step `epsilon`; scale: s['scale'] or None (1)."""
        C, p = s['cur'].shape
        eps, scale, beta = _ptr(s.get('eps')), _ptr(s.get('scale')), _ptr(s.get('beta'))
        cur, grad_cur, sigma = s['cur'].data_ptr(), s['gcur'].data_ptr(), self.sigma
        rest = (C, self.chain0, p, self.seed, self._step_ptr(s), s['mom'].data_ptr(), s['q'].data_ptr(), s['kcur'].data_ptr(), st)
        if beta is not None:
            _lib.check(self._L.qn_hmc_begin_t(cur, grad_cur, sigma, eps, scale, beta, *rest), "qn_hmc_begin_t")
        elif eps is not None:
            _lib.check(self._L.qn_hmc_begin_s(cur, grad_cur, sigma, eps, scale, *rest), "qn_hmc_begin_s")
        else:
            _lib.check(self._L.qn_hmc_begin(cur, grad_cur, sigma, self.epsilon, *rest), "qn_hmc_begin")

    def _leap(self, s, last, st):
        """Enqueue the leap call behind a gradient at s['q']; the entry point is chosen as in `_begin`."""
        C, p = s['cur'].shape
        eps, scale, beta = _ptr(s.get('eps')), _ptr(s.get('scale')), _ptr(s.get('beta'))
        grad_q, dtype, sigma = s['gq'].data_ptr(), self.op.qdt, self.sigma
        rest = (int(last), C, p, s['mom'].data_ptr(), s['q'].data_ptr(), s['kprop'].data_ptr(), st)
        if beta is not None:
            _lib.check(self._L.qn_hmc_leap_t(grad_q, dtype, sigma, eps, scale, beta, *rest), "qn_hmc_leap_t")
        elif eps is not None:
            _lib.check(self._L.qn_hmc_leap_s(grad_q, dtype, sigma, eps, scale, *rest), "qn_hmc_leap_s")
        else:
            _lib.check(self._L.qn_hmc_leap(grad_q, dtype, sigma, self.epsilon, *rest), "qn_hmc_leap")

    def _step(self, s, nmcmc):
        """Enqueue one HMC step on the current stream (reads slot s['par'] of the scalars, writes the other)."""
        st = self._stream()
        C, p = s['cur'].shape
        self._begin(s, st)
        for j in range(self.L):
            qc = s['q'] if s['qc'] is None else s['qc'].copy_(s['q'])          # float32 operator: cast the positions
            self.op.sse_grad(qc, out=(s['sse'], s['gq']))
            self._fold(s, s['q'], s['sse'], s['gq'])                         # (the float64 positions, also under a float32 operator)
            self._leap(s, j == self.L - 1, st)
        g64 = s['gq'] if s['g64'] is None else s['g64'].copy_(s['gq'])
        args = (s['q'].data_ptr(), g64.data_ptr(), s['sse'].data_ptr(), s['kcur'].data_ptr(), s['kprop'].data_ptr(),
                self.sigma, self.op.N, C, self.chain0, p, nmcmc, self.seed, s['cur'].data_ptr(), s['gcur'].data_ptr(),
                s['cur_lp'].data_ptr(), s['best'].data_ptr(), s['best_lp'].data_ptr(), _ptr(s['chain']), s['lps'].data_ptr(),
                s['alphas'].data_ptr(), s['nacc'].data_ptr(), s['step'].data_ptr(), s['par'])
        if s.get('beta') is not None:
            _lib.check(self._L.qn_hmc_accept_t(*args, s['beta'].data_ptr(), st), "qn_hmc_accept_t")
        else:
            _lib.check(self._L.qn_hmc_accept(*args, st), "qn_hmc_accept")
        s['par'] ^= 1

    def _fold(self, s, W, sse, grad):
        """Enqueue the ONE fold behind a gradient call at W, from what the state holds: s['kappa'] (a sampled noise level, the
        weight prior in the same launch), else s['lam'] (per-group precisions: the current slot of lam / c0), else the scalar
        prior, else nothing."""
        if s.get('kappa') is not None:
            self.op.noise_fold(W, s['kappa'][s['npar']], s['d0'][s['npar']], *self._noise_prior(s), sse=sse, grad=grad)
        elif s.get('lam') is not None:
            self.op.prior_fold_g(W, s['lam'][s['hpar']], s['c0'][s['hpar']], s['seg'], sse=sse, grad=grad)
        elif self._prior is not None:
            self.op.prior_fold(W, *self._prior, sse=sse, grad=grad)

    def _swap_step(self, s, nmcmc):
        """Enqueue exchange round s['round'] after the step just decided (and its adaptation); like `_adapt_step` it reads that
        step from slot s['par'] of the step counter, and it writes the other slot of every scalar: the parity flips.  The
        replica ids have a parity of their own (only exchange rounds write them): that of the round."""
        C, p = s['cur'].shape
        _lib.check(self._L.qn_pt_swap(
            s['cur'].data_ptr(), s['gcur'].data_ptr(), s['cur_lp'].data_ptr(), s['best_lp'].data_ptr(), s['lps'].data_ptr(),
            s['chain'].data_ptr() if s['chain'] is not None else None, s['beta'].data_ptr(), s['rid'].data_ptr(),
            s['rep'].data_ptr(), s['swap_acc'].data_ptr(), s['swap_try'].data_ptr(), s['step'].data_ptr(), self._ladder.size,
            s['round'], s['rep'].shape[1] - 1, C, self.chain0, p, nmcmc, self.seed, s['par'], s['round'] & 1, self._stream()),
            "qn_pt_swap")
        s['par'] ^= 1
        s['round'] += 1

    def _hyper_step(self, s, nmcmc):
        """Enqueue Gibbs round s['hround'] of the group precisions after the step just decided (and its adaptation): like
        `_swap_step` it reads slot s['par'] of the scalars and writes the other, and slot s['hpar'] of lam / c0 likewise."""
        a0, b0 = s['hyper']
        self.op.hyper_gibbs(s['cur'], s['gcur'], s['cur_lp'], s['best_lp'], s['lps'], s['lam'], s['c0'], s['seg'], s['taus'],
                            s['step'], self.sigma, a0, b0, s['hround'], self.chain0, self.seed, s['par'], s['hpar'])
        s['par'] ^= 1
        s['hpar'] ^= 1
        s['hround'] += 1

    @staticmethod
    def _noise_prior(s):
        """(lam [C, G], c0 [C], seg [G + 1]) qn_noise_fold / qn_noise_gibbs read: the current slot of a hyper-prior, else the
        one-group arrays of a scalar prior (s['plam']), else three None (G = 0)."""
        if s.get('lam') is not None:
            return s['lam'][s['hpar']], s['c0'][s['hpar']], s['seg']
        if s.get('plam') is not None:
            return s['plam'], s['pc0'], s['pseg']
        return None, None, None

    def _noise_step(self, s, nmcmc):
        """Enqueue Gibbs round s['nround'] of the noise level after the step just decided, its adaptation and its hyper round:
        like `_hyper_step` it reads slot s['par'] of the scalars and writes the other, and slot s['npar'] of kappa / d0 likewise."""
        a0, b0, n = s['noise']
        self.op.noise_gibbs(s['cur'], s['gcur'], s['cur_lp'], s['best_lp'], s['lps'], s['kappa'], s['d0'], *self._noise_prior(s),
                            s['sig'], s['step'], self.sigma, a0, b0, n, s['nround'], self.chain0, self.seed, s['par'], s['npar'])
        s['par'] ^= 1
        s['npar'] ^= 1
        s['nround'] += 1

    def _gibbs_step(self, s, nmcmc, a=None):
        """A step and what follows it, in the one order there is: accept, adapt (a: the step's entry of `warmup_plan`, None after
        the warm-up), exchange round, hyper round, noise round -- a round after every s['severy']-th / s['hevery']-th /
        s['nevery']-th step (absent or 0: never; the constructor refuses a ladder together with a Gibbs round)."""
        self._step(s, nmcmc)
        if a is not None:
            self._adapt_step(s, nmcmc, a)
        n = s['nstep'] = s.get('nstep', 0) + 1
        if s.get('severy') and n % s['severy'] == 0:
            self._swap_step(s, nmcmc)
        if s.get('hevery') and n % s['hevery'] == 0:
            self._hyper_step(s, nmcmc)
        if s.get('nevery') and n % s['nevery'] == 0:
            self._noise_step(s, nmcmc)

    def _adapt_step(self, s, nmcmc, a):
        """Enqueue the adaptation after a warm-up step (a: that step's entry of `warmup_plan`); reads the step just decided
        from the slot of the step counter the accept call wrote, which is s['par'] after `_step`."""
        C, p = s['cur'].shape
        _lib.check(self._L.qn_hmc_adapt(s['cur'].data_ptr(), s['alphas'].data_ptr(), nmcmc, s['step'].data_ptr(), s['par'], C, p,
                                        a['m'], self.target_accept, int(a['collect']), int(a['finish']), int(a['freeze']),
                                        a['n'], s['da'].data_ptr(), s['eps'].data_ptr(), _ptr(s['wmean']), _ptr(s['wm2']),
                                        _ptr(s['scale']), self._stream()), "qn_hmc_adapt")

    def _clone(self, op, chain0):
        return DeviceHMC(op, self.sigma, self.epsilon, self.L, self.seed, chain0, self.use_graph, groups=1, adapt=self.adapt,
                         target_accept=self.target_accept, adapt_mass=self.adapt_mass, ladder=self._ladder,
                         beta_min=self.beta_min, swap_every=self.swap_every, priorsigma=self.priorsigma,
                         hyperprior=self._hyper, noiseprior=self._noise)

    def _check_groups(self, nmcmc, C, p):
        if self._ladder is not None:
            G = self._ngroups(C)
            for g in range(G + 1):
                check_whole_ladders(self._ladder.size, None, C * g // G)

    def _extra_keys(self, nmcmc):
        f64, keys = np.float64, {}
        rounds = lambda every: nmcmc // every if every else 0
        if self.adapt:
            mass = any(a['finish'] for a in warmup_plan(self.adapt, self.adapt_mass))
            keys.update(epsilon=((), f64), mass_scale=((self.op.p,), f64) if mass else None, nwarm=self.adapt)
        if self._ladder is not None:
            keys.update(beta=((), f64), swap_rate=((), f64), replica=((rounds(int(self.swap_every)) + 1,), np.int32))
        if self._hyper is not None:
            keys['tau'] = ((rounds(self._hyper['every']) + 1, len(self._seg) - 1), f64)
        if self._noise is not None:
            keys['sigma'] = ((rounds(self._noise['every']) + 1,), f64)
        return keys

    def _hyper_state(self, C, nmcmc):
        """The run state of a hyper-prior (empty without one): per chain and group lam = sigma^2 tau and the constant c0,
        double-buffered; the group bounds; the trace of the precisions."""
        if self._hyper is None:
            return {}
        dev, f64 = self.dev, torch.float64
        hp, G = self._hyper, len(self._seg) - 1
        every = hp['every']
        tau = np.tile(initial_tau(hp, G, self.priorsigma), (C, 1))
        lam, c0 = fold_constants_g(self.sigma, tau, self._seg, hp['a0'], hp['b0'])
        lam, c0 = torch.as_tensor(lam, dtype=f64, device=dev), torch.as_tensor(c0, dtype=f64, device=dev)
        hs = {'lam': torch.stack([lam, lam]), 'c0': torch.stack([c0, c0]), 'seg': torch.as_tensor(self._seg, device=dev),
              'taus': torch.empty(C, (nmcmc // every if every else 0) + 1, G, dtype=f64, device=dev), 'hpar': 0, 'hround': 0,
              'hyper': (hp['a0'], hp['b0']), 'hevery': every}
        hs['taus'][:, 0] = torch.as_tensor(tau, dtype=f64, device=dev)
        return hs

    def _noise_state(self, C, p, nmcmc):
        """The run state of a noise prior (empty without one): per chain kappa = sigma^2 / s2 and the constant d0,
        double-buffered; the trace of the noise level; without a hyper-prior, a scalar weight prior as one group on the device."""
        if self._noise is None:
            return {}
        dev, f64 = self.dev, torch.float64
        npr, n = self._noise, self.op.N * self.op.Y.shape[1]
        every = npr['every']
        sig0 = self.sigma if npr['sigma_init'] is None else npr['sigma_init']
        kappa, d0 = fold_constants_n(self.sigma, np.full(C, sig0 * sig0), n, self.op.N, npr['a0'], npr['b0'])
        kappa, d0 = torch.as_tensor(kappa, dtype=f64, device=dev), torch.as_tensor(d0, dtype=f64, device=dev)
        ns = {'kappa': torch.stack([kappa, kappa]), 'd0': torch.stack([d0, d0]), 'npar': 0, 'nround': 0,
              'sig': torch.empty(C, (nmcmc // every if every else 0) + 1, dtype=f64, device=dev),
              'noise': (npr['a0'], npr['b0'], n), 'nevery': every}
        ns['sig'][:, 0] = sig0
        if self._hyper is None and self._prior is not None:
            ns.update(plam=torch.full((C, 1), self._prior[0], dtype=f64, device=dev),
                      pc0=torch.full((C,), self._prior[1], dtype=f64, device=dev),
                      pseg=torch.as_tensor([0, p], dtype=torch.int64, device=dev))
        return ns

    def _ladder_state(self, C, nmcmc):
        """The run state of a ladder (empty without one): per-chain inverse temperature and step size epsilon / sqrt(beta_r);
        the replica trace, which starts at the global chain ids; the exchange counters."""
        if self._ladder is None:
            return {}
        dev, f64 = self.dev, torch.float64
        R, nrounds = self._ladder.size, nmcmc // int(self.swap_every)
        beta = torch.as_tensor(np.tile(self._ladder, C // R), dtype=f64, device=dev)
        ids = torch.arange(self.chain0, self.chain0 + C, dtype=torch.int32, device=dev)
        ls = {'beta': beta, 'rid': torch.stack([ids, ids]), 'rep': torch.zeros(C, nrounds + 1, dtype=torch.int32, device=dev),
              'swap_acc': torch.zeros(C, dtype=torch.int64, device=dev), 'swap_try': torch.zeros(C, dtype=torch.int64, device=dev),
              'round': 0, 'eps': self.epsilon / torch.sqrt(beta), 'severy': int(self.swap_every)}
        ls['rep'][:, 0] = ids
        return ls

    def _run_gen(self, nmcmc, param_ini, store_chain=True, verbose=False, chain_out=None):
        """The run as a generator: yields after every enqueued step (pair of steps under a graph); nothing is awaited."""
        check_adapt_args(self.adapt, self.target_accept, nmcmc)
        dev, f64 = self.dev, torch.float64
        cur = torch.as_tensor(param_ini, dtype=f64, device=dev).clone().reshape(-1, self.op.p)
        C, p = cur.shape
        if self._ladder is not None:
            check_whole_ladders(self._ladder.size, C, self.chain0)
        nk = int(self._L.qn_hmc_parts(p))
        f32op = self.op.tdt != f64
        sse0, g0 = self.op.sse_grad(cur if not f32op else cur.to(self.op.tdt))
        extra = dict(self._hyper_state(C, nmcmc), **self._noise_state(C, p, nmcmc), nstep=0)
        self._fold(extra, cur, sse0, g0)                                      # the initial state's, from slot 0 of every pair
        s = self._new_state(cur, sse0, nmcmc, store_chain, chain_out)
        s.update(extra)
        s.update(self._ladder_state(C, nmcmc))
        s.update({'gcur': g0.double() if f32op else g0.clone(),
                  'mom': torch.empty(C, p, dtype=f64, device=dev), 'q': torch.empty(C, p, dtype=f64, device=dev),
                  'gq': torch.empty(C, p, dtype=self.op.tdt, device=dev), 'sse': torch.empty(C, dtype=f64, device=dev),
                  'qc': torch.empty(C, p, dtype=self.op.tdt, device=dev) if f32op else None,
                  'g64': torch.empty(C, p, dtype=f64, device=dev) if f32op else None,
                  'kcur': torch.empty(C, nk, dtype=f64, device=dev), 'kprop': torch.empty(C, nk, dtype=f64, device=dev)})
        i = 0
        # a run without rounds (and every run under a graph: the constructor refuses rounds there) takes plain steps
        step = self._gibbs_step if s.get('severy') or s.get('hevery') or s.get('nevery') else self._step
        if self.adapt:
            # warm-up: direct launches, every step followed by its adaptation; afterwards eps / scale are frozen device arrays
            plan = warmup_plan(self.adapt, self.adapt_mass)
            mass = any(a['finish'] for a in plan)
            s['da'] = torch.zeros(C, 4, dtype=f64, device=dev)          # (mu, Hbar, logbar, logeps)
            if self._ladder is None:
                s['eps'] = torch.full((C,), self.epsilon, dtype=f64, device=dev)
                s['da'][:, 0], s['da'][:, 3] = np.log(10 * self.epsilon), np.log(self.epsilon)
            else:
                s['da'][:, 0], s['da'][:, 3] = torch.log(10 * s['eps']), torch.log(s['eps'])
            s['scale'] = torch.ones(C, p, dtype=f64, device=dev) if mass else None
            s['wmean'] = torch.zeros(C, p, dtype=f64, device=dev) if mass else None
            s['wm2'] = torch.zeros(C, p, dtype=f64, device=dev) if mass else None
            for a in plan:
                self._gibbs_step(s, nmcmc, a)
                i += 1
                yield
        if self.use_graph and nmcmc - i >= 4:
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
            while i + 2 <= nmcmc:
                graph.replay()
                i += 2
                yield
                if verbose and nmcmc >= 10 and i % max(2, (nmcmc // 10) // 2 * 2) == 0:
                    print('%d / %d completed, acceptance rate %lg' % (i, nmcmc, float(s['nacc'].double().mean()) / i))
        while i < nmcmc:
            step(s, nmcmc)
            i += 1
            yield
            if verbose and nmcmc >= 10 and (i + 1) % (nmcmc // 10) == 0:
                print('%d / %d completed, acceptance rate %lg' % (i + 1, nmcmc, float(s['nacc'].double().mean()) / i))
        out = self._results(s, nmcmc)
        if self.adapt:
            out.update(epsilon=s['eps'], mass_scale=s['scale'], nwarm=self.adapt)
        if self._ladder is not None:
            out.update(beta=s['beta'], swap_rate=s['swap_acc'].double() / s['swap_try'].double(), replica=s['rep'])
        if self._hyper is not None:
            out['tau'] = s['taus']
        if self._noise is not None:
            out['sigma'] = s['sig']
        return out
