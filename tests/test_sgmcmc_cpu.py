"""CPU: the contract of the stochastic-gradient samplers (quinn_amd/mcmc/sgmcmc.py) -- the numpy Philox restatement against
the published known answer, the minibatch rows, the step-size schedule, the update's stationary covariance on a Gaussian
target, the argument refusals, and the refusal of a host engine."""
import numpy as np
import pytest
import torch
from scipy import stats

from quinn_amd import _lib
from quinn_amd.mcmc import sgmcmc as sg


def test_philox_restatement_gives_the_random123_known_answer():
    # Random123 kat_vectors, philox4x32-10 with a zero counter and a zero key
    got = sg.philox4x32(0, 0, np.zeros(1, dtype=np.uint64))[0]
    assert [int(w) for w in got] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    # vectorised over the counter; a word depends on key, stream and counter
    many = sg.philox4x32(7, 3, np.arange(5, dtype=np.uint64))
    assert many.shape == (5, 4) and many.dtype == np.uint32
    assert np.array_equal(many[2], sg.philox4x32(7, 3, np.array([2], dtype=np.uint64))[0])
    for other in (sg.philox4x32(8, 3, np.arange(5)), sg.philox4x32(7, 4, np.arange(5)), sg.philox4x32(7, 3, np.arange(5) + 5)):
        assert not np.array_equal(many, other)
    # the upper halves of seed and stream are key / counter words of their own
    assert not np.array_equal(sg.philox4x32(7 + (1 << 32), 3, np.arange(5)), many)
    assert not np.array_equal(sg.philox4x32(7, 3 + (1 << 32), np.arange(5)), many)


def test_counter_layout():
    assert int(sg.ctr_of(5, 4, 9)) == (5 << 40) | (4 << 36) | 9
    assert int(sg.ctr_of(1, 5, (1 << 36) + 2)) == (1 << 40) | (5 << 36) | 2


def test_minibatch_rows_are_in_range_and_keyed_by_seed_step_chain():
    for N, Nb in ((1, 9), (7, 5), (4096, 257), (100003, 1000)):
        r = sg.minibatch_rows(3, 11, 2, N, Nb)
        assert r.dtype == np.int32 and r.shape == (Nb,)
        assert r.min() >= 0 and r.max() < N
    a = sg.minibatch_rows(3, 11, 2, 4096, 64)
    assert np.array_equal(a, sg.minibatch_rows(3, 11, 2, 4096, 64))
    # a prefix does not depend on the batch size: entry j is word j & 3 of block j >> 2
    assert np.array_equal(a[:13], sg.minibatch_rows(3, 11, 2, 4096, 13))
    assert not np.array_equal(a, sg.minibatch_rows(4, 11, 2, 4096, 64))       # seed
    assert not np.array_equal(a, sg.minibatch_rows(3, 12, 2, 4096, 64))       # step
    assert not np.array_equal(a, sg.minibatch_rows(3, 11, 3, 4096, 64))       # chain


def test_minibatch_rows_are_uniform():
    N, n = 7, 70000
    counts = np.bincount(sg.minibatch_rows(1, 0, 0, N, n), minlength=N)
    chi2 = np.sum((counts - n / N) ** 2 / (n / N))
    assert chi2 < stats.chi2.isf(1e-6, N - 1), (chi2, counts)


def test_step_size_schedule_and_noise_mask():
    eta0, K = 0.3, 8
    assert sg.step_size(5, eta0) == eta0 and sg.noise_on(5) is True
    eta = np.array([sg.step_size(t, eta0, 'cyclic', K) for t in range(3 * K)])
    assert np.all(eta[::K] == eta0)                                           # a cycle starts at eta0
    for c in range(3):
        assert np.all(np.diff(eta[c * K:(c + 1) * K]) < 0)                    # and decreases inside the cycle
    assert eta[K - 1] > 0 and np.all(eta > 0)                                 # the last step of a cycle still moves
    np.testing.assert_allclose(eta[K // 2], eta0 / 2, rtol=1e-15)
    on = [bool(sg.noise_on(t, K, 0.5)) for t in range(2 * K)]
    assert on == ([False] * 4 + [True] * 4) * 2                               # flips at explore_frac of the cycle
    assert all(sg.noise_on(t, K, 0.0) for t in range(K))
    assert [bool(sg.noise_on(t, 4, 0.3)) for t in range(4)] == [False, False, True, True]


def test_sg_step_formula():
    rs = np.random.RandomState(0)
    th, v, g, z = rs.randn(4, 5), rs.randn(4, 5), rs.randn(4, 5), rs.randn(4, 5)
    eta, alpha, gs, T = 0.01, 0.2, sg.grad_scale(100, 10, 0.5), 0.7
    assert gs == (100 / 10) * 0.5 / 0.25
    t1, v1 = sg.sg_step(th, v, g, z, eta, alpha, gs, T)
    np.testing.assert_allclose(v1, (1 - alpha) * v - eta * gs * g + np.sqrt(2 * alpha * eta * T) * z, rtol=1e-14)
    np.testing.assert_allclose(t1, th + v1, rtol=0, atol=0)
    t2, v2 = sg.sg_step(th, None, g, z, eta, 1.0, gs, T, on=False)            # SGLD never reads v; masked noise
    np.testing.assert_allclose(t2, th - eta * gs * g, rtol=1e-14)


def test_sgld_on_a_gaussian_target_has_the_ula_covariance():
    """Full-batch SGLD on U = theta^T Lambda theta / 2: n independent chains from 0, each long enough to forget its start
    ((1 - eta lambda_min)^400 < 1e-30), give n independent draws from the stationary law N(0, ula_cov).  With the known
    zero mean, S = X^T X / n has Var(S_ij) = (S_ii S_jj + S_ij^2) / n for Gaussian draws: the bound is 5 of those standard
    errors (derived from n, not from what the code gives).  eta lambda_max = 0.5 makes the discretisation visible: the exact
    posterior inv(Lambda) is 1 / (1 - 0.25) = 1.33 x smaller along the stiff direction, some 30 standard errors away."""
    Lam = np.array([[2.0, 0.6], [0.6, 1.0]])
    lmax = np.linalg.eigvalsh(Lam).max()
    eta, n, nsteps = 0.5 / lmax, 40000, 400
    rs = np.random.RandomState(5)
    th = np.zeros((n, 2))
    for _ in range(nsteps):
        th, _ = sg.sg_step(th, None, th @ Lam, rs.randn(n, 2), eta, 1.0, 1.0)
    want = sg.ula_cov(Lam, eta)
    np.testing.assert_allclose(want, np.linalg.inv(Lam - eta * Lam @ Lam / 2), rtol=1e-14)
    S = th.T @ th / n
    se = np.sqrt((np.outer(np.diag(want), np.diag(want)) + want ** 2) / n)
    assert np.all(np.abs(S - want) < 5 * se), (S, want, se)
    assert np.any(np.abs(S - np.linalg.inv(Lam)) > 10 * se)                   # the check can tell the two apart
    assert abs(th.mean()) < 5 * np.sqrt(want.max() / n)


def test_check_sg_args_refusals():
    assert sg.check_sg_args(1e-3) is None
    assert sg.check_sg_args(1e-3, 0.1, 32, 2, 'cyclic', 4, 0.25, 1.0, nmcmc=20) == 10
    assert sg.check_sg_args(1e-3, schedule='cyclic', cycles=3) is None          # K is known once nmcmc is
    for kw in (dict(eta=0.0), dict(eta=-1e-3), dict(eta=float('nan')),
               dict(eta=1e-3, alpha=0.0), dict(eta=1e-3, alpha=1.5), dict(eta=1e-3, alpha=-0.1),
               dict(eta=1e-3, batch=0), dict(eta=1e-3, batch=-4), dict(eta=1e-3, batch=2.5),
               dict(eta=1e-3, thin=0), dict(eta=1e-3, thin=-1),
               dict(eta=1e-3, schedule='cosine'), dict(eta=1e-3, temperature=-1.0),
               dict(eta=1e-3, schedule='cyclic', cycles=0),
               dict(eta=1e-3, schedule='cyclic', explore_frac=1.5),
               dict(eta=1e-3, schedule='cyclic', cycles=6, nmcmc=10),            # 10 // 6 = 1 inner step per cycle
               dict(eta=1e-3, schedule='cyclic', cycles=11, thin=2, nmcmc=10)):  # 20 // 11 = 1
        with pytest.raises(ValueError):
            sg.check_sg_args(**kw)
    assert sg.check_sg_args(1e-3, schedule='cyclic', cycles=5, nmcmc=10) == 2    # 2 inner steps per cycle are enough


def test_c_abi_refuses_bad_arguments_without_a_device():
    _lib.build()
    L = _lib.lib()
    assert L.qn_sg_rows(None, 1, 4, 7, 0, 0, None, 0, None) == -1 and b"qn_sg_rows" in L.qn_last_error()
    one = 0x1000                                                      # never dereferenced: the refusals come first
    ok = dict(theta=one, v=one, grad=one, dtype=_lib.QN_F64, sse=one, sigma=0.1, n_rows=64, n_batch=8, eta0=1e-3, alpha=0.1,
              temperature=1.0, schedule=0, cycle_len=0, explore_frac=0.0, thin=1, final=0, C=2, chain0=0, p=5, nstore=3, seed=1,
              theta_op=None, best=one, best_lp=one, chain=None, lps=one, rows=None, step_ptr=one, parity=0, stream=None)
    for bad in (dict(theta=None), dict(v=None), dict(grad=None), dict(sse=None), dict(sigma=0.0), dict(n_batch=0),
                dict(eta0=0.0), dict(alpha=0.0), dict(alpha=1.5), dict(temperature=-1.0), dict(schedule=2),
                dict(schedule=1, cycle_len=1), dict(schedule=1, cycle_len=4, explore_frac=2.0), dict(thin=0), dict(C=0),
                dict(C=70000), dict(chain0=-1), dict(p=0), dict(nstore=-1), dict(best=None), dict(best_lp=None), dict(lps=None),
                dict(step_ptr=None), dict(parity=2), dict(dtype=5), dict(theta_op=one)):
        args = dict(ok, **bad)
        assert L.qn_sg_step(*args.values()) == -1, bad
        assert b"qn_sg_step" in L.qn_last_error()


def test_host_engine_is_refused_and_names_the_device_engine():
    from quinn_amd.nns.mlp import MLP
    from quinn_amd.solvers.nn_mcmc import DEVICE_ENGINES, NN_MCMC
    from quinn_amd.mcmc.device_sgmcmc import DeviceSGHMC, DeviceSGLD
    assert DEVICE_ENGINES['sgld'] is DeviceSGLD and DEVICE_ENGINES['sghmc'] is DeviceSGHMC
    torch.manual_seed(0)
    s = NN_MCMC(MLP(1, 1, (4,), activ='tanh'), verbose=False)
    x = np.linspace(-1, 1, 8).reshape(-1, 1)
    for sampler in ('sgld', 'sghmc'):
        with pytest.raises(ValueError, match="engine='device'"):
            s.fit(x, np.sin(x), zflag=False, nmcmc=5, param_ini=np.zeros(s.pdim), sampler=sampler,
                  sampler_params={'eta': 1e-4}, engine='host')
