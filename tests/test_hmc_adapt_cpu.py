"""CPU: the warm-up contract of HMC / MALA (quinn_amd/mcmc/adapt.py) -- Stan's window schedule, the host samplers against a
straight-line transcription of the contract written here, adapt=0 against the unadapted sampler, the behaviour of the
adaptation on an analytic Gaussian, and the argument validation of the three C-ABI entry points.  The log-posterior
callables are plain numpy: no GPU."""
import ctypes

import numpy as np
import pytest

from quinn_amd import _lib
from quinn_amd.mcmc.adapt import warmup_plan, warmup_schedule
from quinn_amd.mcmc.hmc import HMC
from quinn_amd.mcmc.mala import MALA

STD = np.array([0.05, 1.0, 20.0])


def _lp(X):
    return -0.5 * np.sum((X / STD) ** 2, axis=1)


def _lpg(X):
    return -X / STD ** 2


def _rngs(seeds):
    return [np.random.RandomState(s) for s in seeds]


def _hmc(**kw):
    h = HMC(**kw)
    h.setLogPostBatch(_lp, _lpg)
    return h


# ------------------------------------------------------------------------------------------------ schedule
def test_warmup_schedule_is_stans():
    assert warmup_schedule(300) == (75, (100, 150, 250))
    assert warmup_schedule(1000) == (75, (100, 150, 250, 450, 950))
    assert warmup_schedule(150) == (75, (100,))
    s = warmup_schedule(60)                                     # 75 + 25 + 50 > 60: 15 % / 75 % / 10 %
    assert s.start == 9 and s.ends == (54,)
    assert warmup_schedule(20) == (3, (18,))
    for n in (0, 1, 10, 19):                                    # step size only
        assert warmup_schedule(n).ends == () and warmup_schedule(n).start == n
    for n in range(20, 1200, 7):                                # every schedule: increasing ends inside the warm-up
        s = warmup_schedule(n)
        assert 0 < s.start < s.ends[0] and list(s.ends) == sorted(set(s.ends)) and s.ends[-1] < n


def test_warmup_plan_counts():
    plan = warmup_plan(300)
    assert len(plan) == 300 and plan[-1]['freeze'] and sum(a['freeze'] for a in plan) == 1
    assert [k + 1 for k, a in enumerate(plan) if a['finish']] == [100, 150, 250]
    assert [plan[k - 1]['n'] for k in (75, 76, 100, 101, 150, 250, 251)] == [0, 1, 25, 1, 50, 100, 0]
    assert [plan[k - 1]['m'] for k in (1, 100, 101, 150, 151, 300)] == [1, 100, 1, 50, 1, 50]
    assert not any(a['collect'] or a['finish'] for a in warmup_plan(300, adapt_mass=False))
    assert [a['m'] for a in warmup_plan(10)] == list(range(1, 11))


# ------------------------------------------------------------------------------------------------ transcription
def _contract_chain(seed, x0, eps0, L, nwarm, nmcmc, delta, adapt_mass=True):
    """One chain, the contract of DESIGN 4.5 line by line (whitened leapfrog, dual averaging, Welford windows)."""
    rng = np.random.RandomState(seed)
    lp = lambda x: float(_lp(x[None])[0])
    g = lambda x: _lpg(x[None])[0]
    sched = warmup_schedule(nwarm) if adapt_mass else warmup_schedule(0)
    p = x0.size
    cur, s, eps = x0.copy(), np.ones(p), eps0
    mu, hbar, logbar, m = np.log(10 * eps0), 0.0, 0.0, 0
    n, mean, M2 = 0, np.zeros(p), np.zeros(p)
    chain = [cur.copy()]
    for k in range(1, nmcmc + 1):
        z = rng.randn(p)
        with np.errstate(over="ignore", invalid="ignore"):
            u = z + (eps / 2) * s * g(cur)
            q = cur + eps * s * u
            for _ in range(L - 1):
                u = u + eps * s * g(q)
                q = q + eps * s * u
            u = u + (eps / 2) * s * g(q)
            mh = np.exp((-lp(cur) + np.sum(z ** 2) / 2) - (-lp(q) + np.sum(u ** 2) / 2))
        if rng.random_sample() < mh:
            cur = q
        chain.append(cur.copy())
        if k <= nwarm:
            m += 1
            a = 0.0 if np.isnan(mh) else min(1.0, mh)
            hbar = (1 - 1 / (m + 10)) * hbar + (delta - a) / (m + 10)
            logeps = mu - np.sqrt(m) / 0.05 * hbar
            eta = m ** -0.75
            logbar = eta * logeps + (1 - eta) * logbar
            eps = np.exp(logeps)
            if sched.ends and sched.start < k <= sched.ends[-1]:
                n += 1
                d = cur - mean
                mean = mean + d / n
                M2 = M2 + d * (cur - mean)
            if k in sched.ends:
                s = np.sqrt((n / (n + 5)) * M2 / (n - 1) + 1e-3 * 5 / (n + 5))
                n, mean, M2 = 0, np.zeros(p), np.zeros(p)
                mu, hbar, logbar, m = np.log(10 * eps), 0.0, 0.0, 0
            if k == nwarm:
                eps = np.exp(logbar)
    return np.array(chain), eps, (s if sched.ends else None)


@pytest.mark.parametrize("nwarm,nmcmc,adapt_mass", [(60, 90, True), (300, 330, True), (12, 30, True), (60, 80, False)])
def test_host_hmc_equals_the_transcribed_contract(nwarm, nmcmc, adapt_mass):
    seeds, L, eps0, delta = [3, 4, 5], 4, 0.3, 0.8
    ini = np.stack([np.random.RandomState(100 + s).randn(3) * STD for s in seeds])
    h = _hmc(epsilon=eps0, L=L, adapt=nwarm, adapt_mass=adapt_mass)
    r = h.run(nmcmc, ini, rngs=_rngs(seeds), verbose=False)
    assert r['nwarm'] == nwarm and r['epsilon'].shape == (3,)
    for c, s in enumerate(seeds):
        chain, eps, scale = _contract_chain(s, ini[c], eps0, L, nwarm, nmcmc, delta, adapt_mass)
        np.testing.assert_allclose(r['chain'][c], chain, rtol=1e-12, atol=0)
        np.testing.assert_allclose(r['epsilon'][c], eps, rtol=1e-12)
        if scale is None:
            assert r['mass_scale'] is None
        else:
            np.testing.assert_allclose(r['mass_scale'][c], scale, rtol=1e-12)
    again = _hmc(epsilon=eps0, L=L, adapt=nwarm, adapt_mass=adapt_mass).run(nmcmc, ini, rngs=_rngs(seeds), verbose=False)
    assert np.array_equal(again['chain'], r['chain']) and np.array_equal(again['epsilon'], r['epsilon'])


def test_host_mala_is_the_contract_with_one_leapfrog_step():
    seeds = [7, 8]
    ini = np.zeros((2, 3))
    m = MALA(epsilon=0.05, adapt=60)
    m.setLogPostBatch(_lp, _lpg)
    assert m.target_accept == 0.574 and _hmc(adapt=5).target_accept == 0.8
    r = m.run(100, ini, rngs=_rngs(seeds), verbose=False)
    for c, s in enumerate(seeds):
        chain, eps, scale = _contract_chain(s, ini[c], 0.05, 1, 60, 100, 0.574)
        np.testing.assert_allclose(r['chain'][c], chain, rtol=1e-12, atol=0)
        np.testing.assert_allclose(r['epsilon'][c], eps, rtol=1e-12)
        np.testing.assert_allclose(r['mass_scale'][c], scale, rtol=1e-12)
    one = MALA(epsilon=0.05, adapt=60)                         # a 1-D start: results lose the chain axis
    one.setLogPostBatch(_lp, _lpg)
    np.random.seed(7)
    r1 = one.run(100, ini[0], verbose=False)
    assert np.array_equal(r1['chain'], r['chain'][0]) and r1['epsilon'] == r['epsilon'][0]
    assert r1['mass_scale'].shape == (3,) and r1['nwarm'] == 60


def test_adapt_zero_is_the_unadapted_sampler_bit_for_bit():
    """HMC(adapt=0) against the sampler as it stood before the warm-up existed, transcribed here."""
    seeds, eps, L, nmcmc = [11, 12, 13], 0.04, 3, 60
    ini = np.stack([np.random.RandomState(200 + s).randn(3) * STD for s in seeds])
    r = _hmc(epsilon=eps, L=L, adapt=0).run(nmcmc, ini, rngs=_rngs(seeds), verbose=False)
    assert set(r) == {'chain', 'mapparams', 'maxpost', 'accrate', 'logpost', 'alphas'}
    rngs = _rngs(seeds)
    cur, cur_U = ini.copy(), -_lp(ini)
    for i in range(nmcmc):
        q = cur.copy()
        mom = np.stack([rngs[c].randn(3) for c in range(3)])
        k_cur = np.array([np.sum(np.square(mom[c])) / 2 for c in range(3)])
        mom += eps * _lpg(q) / 2
        for j in range(L):
            q += eps * mom
            if j != L - 1:
                mom += eps * _lpg(q)
        mom += eps * _lpg(q) / 2
        k_prop = np.array([np.sum(np.square(mom[c])) / 2 for c in range(3)])
        prop_U = -_lp(q)
        mh = np.exp((cur_U + k_cur) - (prop_U + k_prop))
        take = np.array([rg.random_sample() for rg in rngs]) < mh
        cur = np.where(take[:, None], q, cur)
        cur_U = np.where(take, prop_U, cur_U)
        assert np.array_equal(r['chain'][:, i + 1], cur) and np.array_equal(r['alphas'][:, i + 1], mh)
    with pytest.raises(ValueError):
        _hmc(adapt=10).run(5, ini, rngs=_rngs(seeds), verbose=False)
    with pytest.raises(ValueError):
        _hmc(adapt=10, target_accept=1.5)
    with pytest.raises(ValueError):
        _hmc(adapt=-1)


# ------------------------------------------------------------------------------------------------ behaviour
SEEDS = list(range(32))
NWARM, NSAMP, LSTEPS = 300, 600, 8


def _adapted(eps0, adapt_mass):
    r = _hmc(epsilon=eps0, L=LSTEPS, adapt=NWARM, adapt_mass=adapt_mass).run(NWARM + NSAMP, np.zeros((32, 3)), rngs=_rngs(SEEDS),
                                                                             verbose=False)
    ch = r['chain'][:, NWARM:]
    acc = (ch[:, 1:] != ch[:, :-1]).any(axis=2).mean(axis=1)          # per chain, sampling phase
    return r, acc


def _bar(lo, hi):
    """A bar from a measured range: the worst observed values widened by one third of the observed spread."""
    return lo - (hi - lo) / 3, hi + (hi - lo) / 3


@pytest.mark.parametrize("eps0", [1.0, 1e-4])
def test_adaptation_recovers_from_a_bad_step_size(eps0):
    """Gaussian target with stds (0.05, 1, 20), 32 chains (seeds 0..31) from the mode, 300 warm-up + 600 sampling steps, L = 8,
    target acceptance 0.8.  eps0 = 1.0 is 10 x the stability limit 2 * 0.05: the fixed-step chain accepts nothing (asserted).
    Measured over the 32 chains (sampling-phase acceptance per chain; mass_scale / std over chains and parameters):
        eps0 = 1.0 : acceptance 0.8783 .. 0.9750 (mean 0.936), mass_scale / std 0.6468 .. 1.3011, epsilon 0.6446 .. 0.9484
        eps0 = 1e-4: acceptance 0.8750 .. 0.9783 (mean 0.942), mass_scale / std 0.7213 .. 1.2582, epsilon 0.6563 .. 1.0538
    (the fixed-L resonance on a Gaussian overshoots the target of 0.8).  The bars are these ranges widened by a third of
    their width on each side: a broken recurrence (no shrinking, a wrong window, a variance instead of a standard deviation)
    lands far outside, another seed does not."""
    measured = {1.0: ((0.8783, 0.9750), (0.6468, 1.3011), (0.6446, 0.9484)),
                1e-4: ((0.8750, 0.9783), (0.7213, 1.2582), (0.6563, 1.0538))}[eps0]
    if eps0 == 1.0:
        fixed = _hmc(epsilon=eps0, L=LSTEPS).run(200, np.zeros((32, 3)), rngs=_rngs(SEEDS), verbose=False)
        assert np.all(fixed['accrate'] == 0.0)
    r, acc = _adapted(eps0, True)
    ratio = r['mass_scale'] / STD
    print("eps0", eps0, "acceptance", acc.min(), acc.mean(), acc.max(), "ratio", ratio.min(), ratio.max(), "epsilon",
          r['epsilon'].min(), r['epsilon'].max())
    for got, (lo, hi) in zip((acc, ratio, r['epsilon']), measured):
        blo, bhi = _bar(lo, hi)
        assert blo <= got.min() and got.max() <= bhi, (got.min(), got.max(), blo, bhi)
    assert r['nwarm'] == NWARM and np.all(np.isfinite(r['chain']))
    # the samples after the warm-up have the target's spread in every coordinate (32 x 600 draws; 15 %)
    sd = r['chain'][:, NWARM + 1:].reshape(-1, 3).std(axis=0)
    np.testing.assert_allclose(sd, STD, rtol=0.15)


def test_step_size_alone_settles_at_the_smallest_scale():
    """adapt_mass=False from eps0 = 1: the identity mass leaves the smallest std (0.05) in charge of the step.  Measured over
    the 32 chains: epsilon 0.0577 .. 0.0654, sampling-phase acceptance 0.8250 .. 0.9517; bars widened by a third as above."""
    r, acc = _adapted(1.0, False)
    print("epsilon", r['epsilon'].min(), r['epsilon'].max(), "acceptance", acc.min(), acc.mean(), acc.max())
    assert r['mass_scale'] is None
    for got, (lo, hi) in ((r['epsilon'], (0.0577, 0.0654)), (acc, (0.8250, 0.9517))):
        blo, bhi = _bar(lo, hi)
        assert blo <= got.min() and got.max() <= bhi, (got.min(), got.max(), blo, bhi)


def test_a_diverged_trajectory_shrinks_the_step_and_does_not_poison_the_state():
    """Acceptance NaN counts as 0: the dual-averaging state stays finite and moves exactly as for a = 0."""
    from quinn_amd.mcmc.adapt import HostAdaptation
    a, b = HostAdaptation(2, 3, 0.5, 20, 0.8), HostAdaptation(2, 3, 0.5, 20, 0.8)
    cur = np.zeros((2, 3))
    for k in range(1, 6):
        a.update(k, np.array([np.nan, np.inf]), cur)
        b.update(k, np.array([0.0, 1.0]), cur)
        assert np.array_equal(a.eps, b.eps) and np.all(np.isfinite(a.eps))
    assert a.eps[0] < 0.5 < a.eps[1]


# ------------------------------------------------------------------------------------------------ plumbing
def test_result_plumbing_carries_the_new_keys():
    from quinn_amd.parallel import adapt_keys, empty_results, gather_results
    assert set(empty_results(5, 3)) == {'chain', 'mapparams', 'maxpost', 'accrate', 'logpost', 'alphas'}
    e = empty_results(30, 3, *adapt_keys(25, True))
    assert e['epsilon'].shape == (0,) and e['mass_scale'].shape == (0, 3) and e['nwarm'] == 25
    assert empty_results(30, 3, *adapt_keys(10, True))['mass_scale'] is None          # no window below 20 steps
    assert empty_results(30, 3, *adapt_keys(25, False))['mass_scale'] is None
    r = _hmc(epsilon=0.05, L=2, adapt=25).run(30, np.zeros((2, 3)), rngs=_rngs([1, 2]), verbose=False)
    g = gather_results(r, 2)
    assert g['nwarm'] == 25 and g['epsilon'].shape == (2,) and g['mass_scale'].shape == (2, 3)
    assert np.array_equal(g['chain'], r['chain'])


def test_solver_refuses_more_warmup_than_steps():
    from quinn_amd.nns.mlp import MLP
    from quinn_amd.solvers.nn_mcmc import NN_MCMC
    s = NN_MCMC(MLP(1, 1, (4,), activ="tanh"), verbose=False)
    x = np.zeros((8, 1))
    for engine in ("host", "device"):
        with pytest.raises(ValueError, match="adapt"):
            s.fit(x, x, zflag=False, nmcmc=20, param_ini=np.zeros(s.pdim), sampler="hmc",
                  sampler_params={"L": 2, "epsilon": 0.01, "adapt": 21}, engine=engine)


# ------------------------------------------------------------------------------------------------ C ABI
def test_entry_points_reject_bad_arguments():
    _lib.build()
    L = _lib.lib()
    EINVAL = -1
    one = ctypes.c_void_p(8)            # a non-null placeholder pointer; never dereferenced: validation fails first
    ok_begin = [one, one, 0.1, one, None, 2, 0, 5, 1, one, one, one, one, None]
    for pos, bad in ((0, None), (1, None), (2, 0.0), (3, None), (5, 0), (5, 65536), (6, -1), (7, 0), (9, None), (10, None),
                     (11, None), (12, None)):
        args = list(ok_begin)
        args[pos] = bad
        assert L.qn_hmc_begin_s(*args) == EINVAL, pos
    assert b"qn_hmc_begin_s" in L.qn_last_error()
    ok_leap = [one, 0, 0.1, one, None, 1, 2, 5, one, one, one, None]
    for pos, bad in ((0, None), (1, 3), (2, -1.0), (3, None), (6, 0), (6, 65536), (7, 0), (8, None), (9, None), (10, None)):
        args = list(ok_leap)
        args[pos] = bad
        assert L.qn_hmc_leap_s(*args) == EINVAL, pos
    assert b"qn_hmc_leap_s" in L.qn_last_error()
    # cur, alphas, nmcmc, step_ptr, parity, C, p, m, target, collect, finish, freeze, n, da, eps, mean, m2, scale, stream
    ok_adapt = [one, one, 10, one, 0, 2, 5, 1, 0.8, 1, 1, 0, 2, one, one, one, one, one, None]
    for pos, bad in ((0, None), (1, None), (2, 0), (3, None), (4, 2), (5, 0), (5, 65536), (6, 0), (7, 0), (8, 0.0), (8, 1.0),
                     (11, 1), (12, 1), (13, None), (14, None), (15, None), (16, None), (17, None)):
        args = list(ok_adapt)
        args[pos] = bad
        assert L.qn_hmc_adapt(*args) == EINVAL, pos
    assert b"qn_hmc_adapt" in L.qn_last_error()
    collect_only = list(ok_adapt)
    collect_only[10], collect_only[12] = 0, 0                      # collect with n = 0
    assert L.qn_hmc_adapt(*collect_only) == EINVAL
