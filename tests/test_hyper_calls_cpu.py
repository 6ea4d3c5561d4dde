"""CPU: which prior launch `DeviceHMC._step` makes for each shape of the run state, and what `_hyper_step` hands to the Gibbs
round -- recorded on stub objects in the style of test_device_hmc_calls_cpu.py; no device is needed.  With s['lam'] set the step
calls prior_fold_g (on the CURRENT slot of lam / c0) and never prior_fold; without it the recorded sequence is the one recorded
before the hyper-prior existed."""
import pytest

from quinn_amd.mcmc.device_hmc import DeviceHMC

SIGMA, EPSILON, CHAIN0, SEED, NMCMC, N_ROWS, QDT, C, P, STREAM = 0.25, 0.0125, 6, 991, 40, 48, 1, 4, 97, "stream"
NAMES = ["qn_hmc_begin", "qn_hmc_leap", "qn_hmc_accept", "qn_hmc_begin_s", "qn_hmc_leap_s"]
PRIOR = (0.37, -1.25)


class _T:
    """Stands for a device tensor: an address and a shape; indexing gives the slot's address."""

    def __init__(self, addr):
        self.addr, self.shape = addr, (C, P)

    def data_ptr(self):
        return self.addr

    def __getitem__(self, k):
        return _T(self.addr + 0x100 * (k + 1))


class _Lib:
    def __init__(self, calls):
        for n in NAMES:
            setattr(self, n, lambda *a, _n=n: calls.append((_n, a)) or 0)


def _addr(v):
    return v.addr if isinstance(v, _T) else v


class _Op:
    qdt, N = QDT, N_ROWS

    def __init__(self, calls):
        self.calls = calls

    def sse_grad(self, q, out):
        self.calls.append(("sse_grad", (q.addr, out[0].addr, out[1].addr)))

    def prior_fold(self, W, lam, c0, sse=None, grad=None):
        self.calls.append(("prior_fold", (W.addr, lam, c0, sse.addr, grad.addr)))

    def prior_fold_g(self, W, lam, c0, seg, sse=None, grad=None):
        self.calls.append(("prior_fold_g", (W.addr, lam.addr, c0.addr, seg.addr, sse.addr, grad.addr)))

    def hyper_gibbs(self, *a):
        self.calls.append(("hyper_gibbs", tuple(_addr(v) for v in a)))


class _Engine(DeviceHMC):
    def _stream(self):
        return STREAM


def _engine(L_, prior=None):
    calls = []
    e = _Engine.__new__(_Engine)
    e.sigma, e.epsilon, e.L, e.chain0, e.seed, e._prior = SIGMA, EPSILON, L_, CHAIN0, SEED, prior
    e._L, e.op = _Lib(calls), _Op(calls)
    return e, calls


KEYS = ['cur', 'gcur', 'mom', 'q', 'gq', 'sse', 'kcur', 'kprop', 'cur_lp', 'best', 'best_lp', 'chain', 'lps', 'alphas', 'nacc',
        'step', 'eps', 'scale', 'lam', 'c0', 'seg', 'taus']
A = {k: 0x10000 * (i + 1) for i, k in enumerate(KEYS)}


def _state(par, **extra):
    s = {k: _T(A[k]) for k in KEYS[:16]}
    s.update(par=par, qc=None, g64=None)
    s.update({k: (None if v is None else _T(A[k])) for k, v in extra.items()})
    return s


@pytest.mark.parametrize("prior", [None, PRIOR])
@pytest.mark.parametrize("hpar", [0, 1])
@pytest.mark.parametrize("L_", [1, 3])
@pytest.mark.parametrize("adapt", [False, True])
def test_with_lam_set_the_step_folds_per_group_and_never_the_scalar_prior(prior, hpar, L_, adapt):
    e, calls = _engine(L_, prior)
    s = _state(1, lam=1, c0=1, seg=1, taus=1, **(dict(eps=1, scale=1) if adapt else {}))
    s.update(hpar=hpar, hround=3, hyper=(3.0, 2.0))
    e._step(s, NMCMC)
    sfx = "_s" if adapt else ""
    assert [n for n, _ in calls] == ["qn_hmc_begin" + sfx] + ["sse_grad", "prior_fold_g", "qn_hmc_leap" + sfx] * L_ + ["qn_hmc_accept"]
    slot = 0x100 * (hpar + 1)                                                 # lam[hpar], c0[hpar]: the current slot
    assert all(a == (A['q'], A['lam'] + slot, A['c0'] + slot, A['seg'], A['sse'], A['gq']) for n, a in calls if n == "prior_fold_g")
    assert s['par'] == 0 and s['hpar'] == hpar and s['hround'] == 3          # a step flips the step parity only


@pytest.mark.parametrize("L_", [1, 3])
def test_without_lam_the_recorded_sequence_is_the_one_of_the_scalar_prior_or_of_none(L_):
    for prior, fold in ((None, []), (PRIOR, ["prior_fold"])):
        for extra in (dict(), dict(lam=None)):
            e, calls = _engine(L_, prior)
            s = _state(1, **extra)
            e._step(s, NMCMC)
            assert [n for n, _ in calls] == ["qn_hmc_begin"] + ["sse_grad"] + fold + ["qn_hmc_leap"] + \
                (["sse_grad"] + fold + ["qn_hmc_leap"]) * (L_ - 1) + ["qn_hmc_accept"]
            assert all(a == (A['q'],) + PRIOR + (A['sse'], A['gq']) for n, a in calls if n == "prior_fold")
            assert calls[-1][1] == (A['q'], A['gq'], A['sse'], A['kcur'], A['kprop'], SIGMA, N_ROWS, C, CHAIN0, P, NMCMC, SEED,
                                    A['cur'], A['gcur'], A['cur_lp'], A['best'], A['best_lp'], A['chain'], A['lps'], A['alphas'],
                                    A['nacc'], A['step'], 1, STREAM)


@pytest.mark.parametrize("par,hpar", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_the_gibbs_round_gets_the_state_both_parities_and_the_round_and_flips_them(par, hpar):
    e, calls = _engine(1)
    s = _state(par, lam=1, c0=1, seg=1, taus=1)
    s.update(hpar=hpar, hround=3, hyper=(3.0, 2.0))
    e._hyper_step(s, NMCMC)
    assert calls == [("hyper_gibbs", (A['cur'], A['gcur'], A['cur_lp'], A['best_lp'], A['lps'], A['lam'], A['c0'], A['seg'],
                                      A['taus'], A['step'], SIGMA, 3.0, 2.0, 3, CHAIN0, SEED, par, hpar))]
    assert (s['par'], s['hpar'], s['hround']) == (1 - par, 1 - hpar, 4)
