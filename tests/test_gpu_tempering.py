"""GPU: replica exchange for the device HMC / MALA engines (csrc/qn_hmc_leap.hip, csrc/qn_temper.hip, quinn_amd/mcmc/tempering.py).  The tempered
entry points with beta = 1 against the untempered engines bit for bit; qn_pt_swap against `tempering.swap_round`; exactness of
every rung on a Gaussian target; a bimodal posterior whose second mode only a ladder reaches; the solver."""
import os

import numpy as np
import pytest
import torch

from quinn_amd import _lib
from quinn_amd.mcmc import tempering as pt
from quinn_amd.mcmc.device_hmc import DeviceHMC
from quinn_amd.mcmc.device_mala import DeviceMALA
from quinn_amd.mcmc.sgmcmc import ctr_of, philox4x32
from quinn_amd.ops import BatchedMLP, MLPArch

pytestmark = pytest.mark.gpu
F64 = torch.float64
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _dev(a, dtype=F64):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


# ------------------------------------------------------------------------------------------------ 1. parity with beta = 1
@pytest.mark.parametrize("adapt", [0, 10])
@pytest.mark.parametrize("cls", [DeviceHMC, DeviceMALA])
def test_tempered_entry_points_with_beta_one_equal_the_untempered_engine_bit_for_bit(cls, adapt):
    """(1,16,16,1) tanh, N = 64, C = 8, 20 steps: the engine driven through qn_hmc_begin_t / qn_hmc_leap_t / qn_hmc_accept_t with
    beta = 1 for every chain and no exchange round (the ladder is replaced by ones after the constructor's checks, the first
    round is due after the run) against the same engine without a ladder."""
    rs = np.random.RandomState(4)
    x = rs.rand(64, 1) * 6 - 3
    y = np.sin(x) + 0.1 * rs.randn(64, 1)
    arch = MLPArch((1, 16, 16, 1), "tanh")
    op = BatchedMLP(arch, x, y)
    ini = 0.3 * rs.randn(8, arch.nparams)
    kw = dict(epsilon=0.004, seed=11, adapt=adapt)
    if cls is DeviceHMC:
        kw['L'] = 3
    ref = cls(op, 0.3, **kw).run(20, ini)
    eng = cls(op, 0.3, ladder=2, **kw)
    eng._ladder = np.ones(2)
    eng.swap_every = 10 ** 9
    got = eng.run(20, ini)
    torch.cuda.synchronize()
    keys = ['chain', 'logpost', 'alphas', 'accrate', 'mapparams', 'maxpost'] + (['epsilon'] if adapt else [])
    for k in keys:
        assert np.array_equal(got[k].cpu().numpy(), ref[k].cpu().numpy(), equal_nan=True), k
    acc = ref['accrate'].cpu().numpy()
    assert acc.max() > 0.0                                    # (the comparison is not one of frozen chains)
    assert np.all(got['beta'].cpu().numpy() == 1.0) and got['replica'].shape == (8, 1)
    assert np.all(np.isnan(got['swap_rate'].cpu().numpy()))   # nothing was tried


# ------------------------------------------------------------------------------------------------ 2. the swap kernel
def _swap_inputs(R, K, p, rnd, parity, chain0, seed, t, nmcmc, nrounds, lp=None):
    """Host arrays of one qn_pt_swap call.  The log-posteriors are redrawn (deterministically) until no pair lies within 1e-9 of
    its decision boundary log u = d."""
    C = R * K
    rs = np.random.RandomState(1000 * R + 100 * K + 10 * rnd + 2 * parity + (chain0 > 0) + p)
    beta = np.tile(pt.ladder(R, 0.05), K)
    u = pt.swap_uniform(seed, t, chain0 + np.arange(C))
    lows = np.array([k * R + r for k in range(K) for r in pt.swap_pairs(R, rnd)], dtype=np.int64)
    while lp is None:
        lp = -100.0 + 2.0 * rs.randn(C)
        d = np.array([(beta[c] - beta[c + 1]) * (lp[c + 1] - lp[c]) for c in lows])
        if len(lows) and np.min(np.abs(np.log(u[lows]) - d)) <= 1e-9:      # (R = 2 has no pair in an odd round)
            lp = None
    h = {'cur': rs.randn(C, p), 'gcur': rs.randn(C, p), 'cur_lp': rs.randn(2, C), 'best_lp': rs.randn(2, C),
         'lps': rs.randn(C, nmcmc + 1), 'chain': rs.randn(C, nmcmc + 1, p), 'beta': beta,
         'rid': rs.randint(0, 1000, size=(2, C)).astype(np.int32), 'rep': np.full((C, nrounds + 1), -7, dtype=np.int32),
         'swap_acc': rs.randint(0, 50, size=C).astype(np.int64), 'swap_try': rs.randint(50, 90, size=C).astype(np.int64),
         'step': np.array([-99, -99], dtype=np.int64)}
    h['cur_lp'][parity] = lp
    h['lps'][:, t] = lp
    h['chain'][:, t] = h['cur']
    h['step'][parity] = t
    return h, u, lows


def _swap_call(h, R, rnd, nrounds, chain0, nmcmc, seed, parity, rpar, with_chain=True, with_rep=True):
    L = _lib.lib()
    d = {k: _dev(v, {'rid': torch.int32, 'rep': torch.int32, 'swap_acc': torch.int64, 'swap_try': torch.int64,
                     'step': torch.int64}.get(k, F64)) for k, v in h.items()}
    C, p = h['cur'].shape
    _lib.check(L.qn_pt_swap(d['cur'].data_ptr(), d['gcur'].data_ptr(), d['cur_lp'].data_ptr(), d['best_lp'].data_ptr(),
                            d['lps'].data_ptr(), d['chain'].data_ptr() if with_chain else None, d['beta'].data_ptr(),
                            d['rid'].data_ptr(), d['rep'].data_ptr() if with_rep else None, d['swap_acc'].data_ptr(),
                            d['swap_try'].data_ptr(), d['step'].data_ptr(), R, rnd, nrounds, C, chain0, p, nmcmc, seed, parity,
                            rpar, None), "qn_pt_swap")
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in d.items()}


def _check_swap(h, g, sw, perm, lows, R, rnd, parity, rpar, t, with_chain=True, with_rep=True):
    C = h['cur'].shape[0]
    o = 1 - parity
    assert np.array_equal(g['cur'], h['cur'][perm]) and np.array_equal(g['gcur'], h['gcur'][perm])
    exp_chain = h['chain'].copy()
    if with_chain:
        exp_chain[:, t] = h['cur'][perm]
    assert np.array_equal(g['chain'], exp_chain)              # row t rewritten, every other row untouched
    exp_lps = h['lps'].copy()
    exp_lps[:, t] = h['cur_lp'][parity][perm]
    assert np.array_equal(g['lps'], exp_lps)
    assert np.array_equal(g['cur_lp'][parity], h['cur_lp'][parity]) and np.array_equal(g['cur_lp'][o], h['cur_lp'][parity][perm])
    assert np.array_equal(g['best_lp'][parity], h['best_lp'][parity]) and np.array_equal(g['best_lp'][o], h['best_lp'][parity])
    assert np.array_equal(g['rid'][rpar], h['rid'][rpar]) and np.array_equal(g['rid'][1 - rpar], h['rid'][rpar][perm])
    exp_rep = h['rep'].copy()
    if with_rep:
        exp_rep[:, rnd + 1] = h['rid'][rpar][perm]
    assert np.array_equal(g['rep'], exp_rep)
    low = np.zeros(C, dtype=np.int64)
    low[lows] = 1
    assert np.array_equal(g['swap_try'], h['swap_try'] + low) and np.array_equal(g['swap_acc'], h['swap_acc'] + sw)
    assert g['step'][o] == t and g['step'][parity] == t
    assert np.array_equal(g['beta'], h['beta'])
    unpaired = [c for c in range(C) if c not in lows and c - 1 not in lows]
    assert np.array_equal(perm[unpaired], unpaired)


@pytest.mark.parametrize("R,K,p", [(2, 3, 23), (3, 2, 23), (4, 3, 23), (2, 3, 8513), (3, 2, 8513), (4, 3, 8513)])
def test_swap_kernel_equals_the_host_round(R, K, p):
    """p = 23: odd rows, so every second row's pair accesses are unaligned, one workgroup per chain; p = 8513: nine workgroups
    per chain.  Both rounds, both parities, a launch that starts at global chain 0 and one that starts at chain R."""
    assert _lib.lib().qn_hmc_parts(p) == (1 if p == 23 else 9)
    seed, nmcmc, nrounds = 12345, 5, 4
    outcomes = set()
    for rnd in (0, 1):
        for parity in (0, 1):
            for chain0 in (0, R):
                t = 2 + rnd + parity
                h, u, lows = _swap_inputs(R, K, p, rnd, parity, chain0, seed, t, nmcmc, nrounds)
                lp = h['cur_lp'][parity]
                d = np.array([(h['beta'][c] - h['beta'][c + 1]) * (lp[c + 1] - lp[c]) for c in lows])
                assert np.all(np.abs(np.log(u[lows]) - d) > 1e-9)           # no pair inside the band: decisions must agree
                sw, perm = pt.swap_round(lp, h['beta'], R, rnd, u)
                outcomes |= set(sw[lows].tolist())
                rpar = (parity + (chain0 > 0)) & 1                            # the replica ids' own parity: equal and unequal
                g = _swap_call(h, R, rnd, nrounds, chain0, nmcmc, seed, parity, rpar)
                _check_swap(h, g, sw, perm, lows, R, rnd, parity, rpar, t)
                g2 = _swap_call(h, R, rnd, nrounds, chain0, nmcmc, seed, parity, rpar)
                for k in g:
                    assert np.array_equal(g[k], g2[k]), k                    # equal inputs, equal bits
    assert outcomes == {True, False}


def test_swap_kernel_optional_arrays_and_non_finite_log_posteriors():
    """chain / rep NULL; a NaN lower, a -inf upper and a -inf lower log-posterior (the last one has d = +inf) never swap."""
    R, K, p, seed, nmcmc, nrounds, t = 2, 4, 23, 9, 5, 4, 3
    lp = np.array([np.nan, -3.0, -5.0, -np.inf, -np.inf, -4.0, -90.0, -2.0])      # the last pair always swaps (d = +83.6)
    h, u, lows = _swap_inputs(R, K, p, 0, 0, 0, seed, t, nmcmc, nrounds, lp=lp)
    sw, perm = pt.swap_round(lp, h['beta'], R, 0, u)
    assert sw.tolist() == [False, False, False, False, False, False, True, False]
    g = _swap_call(h, R, 0, nrounds, 0, nmcmc, seed, 0, 1, with_chain=False, with_rep=False)
    o = g['cur_lp'][1]
    assert np.isnan(o[0]) and np.array_equal(o[1:], lp[perm][1:])
    for k in ('cur_lp', 'lps'):                                # (NaN-aware comparison of the rest)
        g[k], h[k] = np.nan_to_num(g[k], nan=123.0), np.nan_to_num(h[k], nan=123.0)
    _check_swap(h, g, sw, perm, lows, R, 0, 0, 1, t, with_chain=False, with_rep=False)


# ------------------------------------------------------------------------------------------------ 3. Gaussian target
def _accept_uniform(seed, step, chains):
    """The accept kernel's uniform of the step taken at device step counter `step` (purpose 2 of the counter layout)."""
    w = philox4x32(seed, 2 * int(step) + 1, ctr_of(np.asarray(chains, dtype=np.uint64), 2, np.zeros(len(chains), dtype=np.uint64)))
    bits = (w[:, 0].astype(np.uint64) << np.uint64(21)) ^ (w[:, 1].astype(np.uint64) >> np.uint64(11))
    return (bits.astype(np.float64) + 0.5) / 9007199254740992.0


@pytest.fixture(scope="module")
def gaussian_run():
    rs = np.random.RandomState(21)
    N, sigma, R, K = 64, 0.5, 4, 16
    x = rs.randn(N, 2)
    y = x @ np.array([[1.0], [-0.5]]) + 0.3 + sigma * rs.randn(N, 1)
    A = np.hstack([x, np.ones((N, 1))])
    w_ols = np.linalg.solve(A.T @ A, A.T @ y)[:, 0]
    cov1 = sigma ** 2 * np.linalg.inv(A.T @ A)
    op = BatchedMLP(MLPArch((2, 1), "identity"), x, y)
    ini = w_ols + 0.1 * rs.randn(R * K, 3)
    seed = 77
    res = DeviceHMC(op, sigma, epsilon=0.02, L=5, seed=seed, adapt=300, ladder=R, beta_min=0.1).run(1500, ini)
    torch.cuda.synchronize()
    res = {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in res.items()}
    return res, w_ols, cov1, R, K, seed


def test_every_rung_samples_its_tempered_gaussian(gaussian_run):
    """Rung r targets N(w_ols, sigma^2 / beta_r (A^T A)^-1).  Per rung and parameter: the mean over the 16 ladders of the
    per-ladder mean (rows 500 ..) within 5 standard errors of the analytic value, the same for the per-ladder variance; the
    standard error is the spread of the 16 independent ladders' values / sqrt(16)."""
    res, w_ols, cov1, R, K, _ = gaussian_run
    beta = pt.ladder(R, 0.1)
    assert np.array_equal(res['beta'], np.tile(beta, K))
    ch = res['chain'][:, 500:, :].reshape(K, R, -1, 3)
    for r in range(R):
        m, v = ch[:, r].mean(axis=1), ch[:, r].var(axis=1, ddof=1)             # [K, 3]
        for j in range(3):
            for name, vals, exact in (("mean", m[:, j], w_ols[j]), ("var", v[:, j], cov1[j, j] / beta[r])):
                se = vals.std(ddof=1) / np.sqrt(K)
                print(f"rung {r} param {j} {name}: {vals.mean():.6g} exact {exact:.6g} ({(vals.mean() - exact) / se:+.2f} se)")
                assert abs(vals.mean() - exact) <= 5 * se, (r, j, name, vals.mean(), exact, se)
    rate = res['swap_rate'].reshape(K, R)
    assert np.all(np.isnan(rate[:, -1])) and np.all(rate[:, :-1] > 0.0) and np.all(rate[:, :-1] < 1.0)


def test_spliced_replica_trajectories_move_only_by_accepted_steps(gaussian_run):
    """Following each replica through the slots `replica` names, consecutive rows differ exactly where the accept kernel's own
    uniform lies below `alphas` of the slot the replica sat in: a swap moves states between slots and changes nothing else."""
    res, _, _, R, K, seed = gaussian_run
    chain, rep, alphas, lps = res['chain'], res['replica'], res['alphas'], res['logpost']
    C, T = rep.shape
    assert T == 1501 and np.array_equal(rep[:, 0], np.arange(C))
    slot = np.argsort(rep, axis=0, kind='stable')             # slot[i, t]: where replica i sits after the rounds of step t
    assert np.array_equal(np.sort(rep, axis=0), np.tile(np.arange(C)[:, None], (1, T)))
    assert np.all(np.abs(np.diff(slot, axis=1)) <= 1) and np.all(slot // R == (np.arange(C) // R)[:, None])
    assert np.any(np.diff(slot, axis=1) != 0)
    tt = np.arange(T)
    X, LP = chain[slot, tt[None, :]], lps[slot, tt[None, :]]  # [C, T, 3], [C, T]
    moved = np.any(X[:, 1:] != X[:, :-1], axis=2)
    for t in range(T - 1):
        s = slot[:, t]
        u = _accept_uniform(seed, t, s)
        with np.errstate(invalid='ignore'):
            take = u < alphas[s, t + 1]
        assert np.array_equal(moved[:, t], take), t
        assert np.array_equal(LP[:, t + 1] != LP[:, t], take), t


# ------------------------------------------------------------------------------------------------ 4. the point of it
def test_cold_chains_visit_both_sign_modes_only_with_a_ladder():
    """w2 tanh(w1 x): (w1, w2) and (-w1, -w2) are the same function, two modes far apart.  All chains start at (1.5, 1)."""
    rs = np.random.RandomState(0)
    x = np.linspace(-2, 2, 32)[:, None]
    y = np.tanh(1.5 * x) + 0.1 * rs.randn(32, 1)
    op = BatchedMLP(MLPArch((1, 1, 1), "tanh", False), x, y)
    R, K = 8, 8
    ini = np.tile([1.5, 1.0], (R * K, 1))
    kw = dict(epsilon=0.01, L=5, seed=3)
    res = DeviceHMC(op, 0.1, ladder=R, beta_min=1e-3, **kw).run(4000, ini)
    w1 = res['chain'][::R, 1001:, 0].cpu().numpy()             # the cold chains
    frac = (w1 < 0).mean(axis=1)
    print("per cold chain:", np.round(frac, 3), "pooled:", frac.mean())
    assert np.all(frac >= 0.05) and np.all(1.0 - frac >= 0.05)
    assert 0.3 <= (w1 < 0).mean() <= 0.7
    trips = pt.round_trips(res['replica'].cpu().numpy(), R).reshape(K, R)
    assert np.all(trips.max(axis=1) >= 1)
    ctl = DeviceHMC(op, 0.1, **kw).run(4000, ini)
    assert (ctl['chain'][:, 1001:, 0].cpu().numpy() < 0).mean() == 0.0


# ------------------------------------------------------------------------------------------------ 5. the solver
def _solver_problem():
    rs = np.random.RandomState(2)
    x = rs.rand(32, 1) * 6 - 3
    return x, np.sin(x) + 0.1 * rs.randn(32, 1)


def test_solver_with_a_ladder_uses_the_cold_chains():
    from quinn_amd.mcmc import diagnostics as diag
    from quinn_amd.nns.mlp import MLP
    from quinn_amd.solvers.nn_mcmc import NN_MCMC
    x, y = _solver_problem()
    torch.manual_seed(0)
    s = NN_MCMC(MLP(1, 1, (8, 8), activ="tanh"), verbose=False)
    ini = 0.1 * np.ones(s.pdim)
    fit = lambda params, C=8, **kw: s.fit(x, y, zflag=False, datanoise=0.3, nmcmc=60, param_ini=ini, sampler='hmc',
                                          sampler_params=params, nchains=C, seeds=list(range(5, 5 + C)), engine='device', **kw)
    fit({'epsilon': 0.01, 'L': 2, 'ladder': 4, 'beta_min': 0.05}, diagnostics=True, diag_nburn=20)
    r = s.mcmc_results
    assert np.array_equal(r['beta'], np.tile(pt.ladder(4, 0.05), 2))
    assert r['swap_rate'].shape == (8,) and r['replica'].shape == (8, 61) and r['replica'].dtype == np.int32
    assert s.samples.shape == (8, 61, s.pdim)
    W = s._ens_weights(6, 20, 'all')
    cold = s.samples[[0, 4]]
    exp = np.concatenate([cold[c][rows] for c, rows in diag.pooled_rows(2, 61, 6, 20)])
    assert np.array_equal(W, exp)
    assert np.array_equal(s.predict_ens(x, nens=6, nburn=20, chain='all'), s._predict_batch_dev(exp, x).double().cpu().numpy())
    assert np.array_equal(s._ens_weights(2, 20, 5), s.samples[5][[20, 40]])        # an int indexes all chains
    for k in ('params', 'logpost'):
        assert s.diagnostics[k]['chain_mean'].shape[0] == 2
    assert s.diagnose(nburn=20)['params']['chain_mean'].shape[0] == 2
    sc = s.score(x, y, noise=0.3, nsam=6, nburn=20, chain='all')
    assert np.isfinite(sc['lppd'])
    with pytest.raises(ValueError):
        fit({'epsilon': 0.01, 'L': 2, 'ladder': 4, 'use_graph': True})
    with pytest.raises(ValueError):
        fit({'epsilon': 0.01, 'L': 2, 'ladder': 3})
    with pytest.raises(ValueError):
        DeviceHMC(s._operator(s.lpinfo), 0.3, ladder=4, groups=4).run(10, np.tile(ini, (8, 1)))    # groups of 2 chains


@pytest.mark.parametrize("case", ["plain", "adapt"])
def test_solver_without_a_ladder_gives_the_parent_commits_results(case):
    """tests/golden/temper_parent_fit.npz: `mcmc_results` of these two fits recorded on an MI355X with the commit before
    replica exchange.  Same keys, same bits."""
    from quinn_amd.nns.mlp import MLP
    from quinn_amd.solvers.nn_mcmc import NN_MCMC
    x, y = _solver_problem()
    torch.manual_seed(0)
    s = NN_MCMC(MLP(1, 1, (8, 8), activ="tanh"), verbose=False)
    params = {'epsilon': 0.01, 'L': 2}
    if case == "adapt":
        params['adapt'] = 10
    s.fit(x, y, zflag=False, datanoise=0.3, nmcmc=30, param_ini=0.1 * np.ones(s.pdim), sampler='hmc', sampler_params=params,
          nchains=4, seeds=[5, 6, 7, 8], engine='device')
    with np.load(os.path.join(GOLDEN, "temper_parent_fit.npz"), allow_pickle=False) as z:
        ref = {k[len(case) + 1:]: z[k] for k in z.files if k.startswith(case + "/")}
    got = {k: v for k, v in s.mcmc_results.items() if v is not None}
    assert set(got) == set(ref)
    for k in ref:
        assert np.array_equal(np.asarray(got[k]), ref[k], equal_nan=True), k
