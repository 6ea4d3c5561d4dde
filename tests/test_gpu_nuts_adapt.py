"""GPU: NUTS's windowed warm-up on the device (qn_nuts_adapt, `DeviceNUTS(adapt_mass=True)`).  One launch with every kind of
chain against the numpy contract, a short run against the host contract driven by the same operator, independence from the way
the chains are split, the untouched default path, the effect on an ill-scaled exact target, and the refusals."""
import numpy as np
import pytest
import torch

from quinn_amd import _lib
from quinn_amd.mcmc import diagnostics as diag
from quinn_amd.mcmc import nuts
from quinn_amd.mcmc import nuts_adapt as na
from quinn_amd.mcmc.adapt import warmup_plan
from quinn_amd.mcmc.device_nuts import DeviceNUTS
from quinn_amd.mcmc.ess import gaussian_posterior
from quinn_amd.ops import BatchedMLP, MLPArch

from test_ess_contract import N as LIN_N, SIGMA as LIN_SIGMA, linear_problem
from test_gpu_nuts import ARCH, KEYS, _ini, _problem, device_momenta
from test_nuts_adapt_contract import REFUSED, adapt_abi_args

pytestmark = pytest.mark.gpu

# (t of the slot read, t of the slot written) of the eight hand-written chains; adapt = 40: no window before step 7, the
# window collects steps 7 .. 36 and ends at 36, step 40 freezes
COUNTERS = [(2, 3),      # 0 ends a step before the windows
            (19, 20),    # 1 inside the window: collect
            (35, 36),    # 2 at the window's end: collect and finish
            (39, 40),    # 3 k = adapt: freeze (with nmcmc = adapt the chain is done: scalars only, no redo)
            (21, 22),    # 4 collect, with a NaN acceptance statistic (counts as 0)
            (44, 45),    # 5 k > adapt
            (10, 10),    # 6 mid-step
            (-1, -1)]    # 7 already done: t = nmcmc in both slots (set per launch)
TOUCHED = (0, 1, 2, 3, 4)


@pytest.mark.parametrize("nmcmc,parity", [(48, 0), (40, 1)])
@pytest.mark.parametrize("p", [1, 7, 2049])                         # 2049: three workgroups per chain, an odd last element
def test_one_launch_against_the_contract(p, nmcmc, parity):
    L, dev, f64 = _lib.lib(), "cuda", torch.float64
    C, adapt, sigma, target = 8, 40, 0.5, 0.8
    assert int(L.qn_hmc_parts(p)) == (3 if p == 2049 else 1)
    rs = np.random.RandomState(p)
    vec = {k: rs.randn(C, p) for k in ('cur', 'ql', 'ul', 'gl', 'q', 'u', 'mean')}
    vec['m2'], vec['scale'] = rs.rand(C, p) * 3, 0.5 + rs.rand(C, p)
    alphas = rs.rand(C, nmcmc + 1) * 1.3                            # (some beyond 1: capped)
    alphas[4, 22] = np.nan
    es = rs.randn(2, C, 12)
    ei = np.zeros((2, C, 8), dtype=np.int64)
    for c, (t0, t1) in enumerate(COUNTERS):
        ei[parity, c, 0], ei[1 - parity, c, 0] = (nmcmc, nmcmc) if c == 7 else (t0, t1)
        ei[parity, c, 1:5] = (2, 3, 1, 6)                           # the old slot: somewhere inside a tree
        ei[1 - parity, c, 3] = 1 if c % 2 else -1                   # the fresh slot: d = i = n_leap = 0 and the new direction
    ei[1 - parity, 6] = ei[parity, 6] + np.array([0, 0, 1, 0, 1, 0, 0, 1])     # (mid-step: the next leaf of the same step)
    ws = np.full((2, C, 4), np.nan)
    ws[parity, :, 0] = np.log(10 * 0.05) + 0.1 * rs.randn(C)
    ws[parity, :, 1], ws[parity, :, 2], ws[parity, :, 3] = 0.05 * rs.randn(C), -3 + 0.3 * rs.randn(C), 0.05 + 0.01 * rs.rand(C)
    plan = na.plan_table(adapt)
    d = {k: torch.as_tensor(v, device=dev) for k, v in dict(vec, alphas=alphas, es=es, ei=ei, ws=ws, plan=plan).items()}
    assert d['plan'].dtype == torch.int32 and d['ei'].dtype == torch.int64 and d['es'].dtype == f64
    _lib.check(L.qn_nuts_adapt(d['cur'].data_ptr(), d['alphas'].data_ptr(), nmcmc, adapt, target, d['plan'].data_ptr(),
                               d['es'].data_ptr(), d['ei'].data_ptr(), parity, C, p, sigma, d['ql'].data_ptr(), d['ul'].data_ptr(),
                               d['gl'].data_ptr(), d['q'].data_ptr(), d['u'].data_ptr(), d['ws'].data_ptr(), d['mean'].data_ptr(),
                               d['m2'].data_ptr(), d['scale'].data_ptr(), None), "qn_nuts_adapt")
    torch.cuda.synchronize()
    h = {k: v.cpu().numpy() for k, v in d.items()}
    bits = lambda a: np.ascontiguousarray(a).view(np.int64)
    # ---- what no chain may lose: the counters, the inputs, and every scalar of es but the fresh slot's eps
    assert np.array_equal(h['ei'], ei) and np.array_equal(h['alphas'], alphas, equal_nan=True) and np.array_equal(h['plan'], plan)
    for k in ('cur', 'ql', 'ul', 'gl'):
        assert np.array_equal(h[k], vec[k]), k
    assert np.array_equal(h['es'][parity], es[parity]) and np.array_equal(h['es'][1 - parity, :, 1:], es[1 - parity, :, 1:])
    assert np.array_equal(bits(h['ws'][parity]), bits(ws[parity]))
    wplan = warmup_plan(adapt, True)
    for c in range(C):
        if c not in TOUCHED:                                       # the contract leaves it alone: every bit, in both slots
            assert np.array_equal(h['es'][:, c], es[:, c]), c
            for k in ('q', 'u', 'mean', 'm2', 'scale'):
                assert np.array_equal(h[k][c], vec[k][c]), (c, k)
            assert np.array_equal(bits(h['ws'][1 - parity, c]), bits(ws[parity, c])), c          # carried over
            continue
        k = COUNTERS[c][1]
        cfg = nuts.nuts_config(sigma, 20, nmcmc, 4, adapt, target, scale=vec['scale'][c])
        old = {'t': COUNTERS[c][0]}
        new = {key: vec[key][c] for key in ('cur', 'ql', 'ul', 'gl', 'q', 'u')}
        new.update(t=k, v=int(ei[1 - parity, c, 3]), n_leap=0, eps=es[1 - parity, c, 0])
        w_in = dict(zip(('mu', 'hbar', 'logbar'), ws[parity, c, :3]), mean=vec['mean'][c], m2=vec['m2'][c])
        got = dict(zip(('mu', 'hbar', 'logbar', 'eps'), h['ws'][1 - parity, c]))
        assert h['es'][1 - parity, c, 0] == got['eps'], c
        # the transcendental scalars, as tests/test_gpu_hmc_adapt.py compares the same formulas of qn_hmc_adapt: 1e-12 relative
        st, w_out, cfg2 = na.nuts_warm_update(old, new, w_in, cfg, wplan, alphas[c])
        for key in ('mu', 'hbar', 'logbar'):
            np.testing.assert_allclose(got[key], w_out[key], rtol=1e-12, atol=0, err_msg=f"{c} {key}")
        np.testing.assert_allclose(got['eps'], st['eps'], rtol=1e-12, atol=0, err_msg=f"{c} eps")
        # everything elementwise, with the device's scalars handed to the contract: bit for bit
        st, w_out, cfg2 = na.nuts_warm_update(old, new, w_in, cfg, wplan, alphas[c], given=got)
        for key, want in (('mean', w_out['mean']), ('m2', w_out['m2']), ('scale', np.broadcast_to(cfg2['scale'], (p,))),
                          ('q', st['q']), ('u', st['u'])):
            assert np.array_equal(h[key][c], want), (c, key)
        s = wplan[k - 1]
        changed = {'mean': s['collect'] or s['finish'], 'm2': s['collect'] or s['finish'], 'scale': s['finish'],
                   'q': k < nmcmc, 'u': k < nmcmc}
        for key, ch in changed.items():                            # (and the contract did something where it should)
            assert ch != np.array_equal(h[key][c], vec[key][c]), (c, key)
        if s['finish']:
            assert not h['mean'][c].any() and not h['m2'][c].any() and (got['hbar'], got['logbar']) == (0.0, 0.0)
    assert wplan[35]['finish'] and wplan[39]['freeze'] and wplan[19]['collect'] and not wplan[2]['collect']


HOST_RUN = dict(epsilon=0.02, max_depth=4, adapt=40, block=8)


def _recorded_run(eng, nm, ini):
    """The run of `eng`, with the warm-up scalars ws = (mu, hbar, logbar, eps) [C, 4] and the step counters [C] the device holds
    after every iteration: `_iter` is followed by a look at the slot it has just written."""
    rec, real = [], eng._iter

    def _iter(s, nmcmc):
        real(s, nmcmc)
        rec.append((s['ws'][s['par']].cpu().numpy(), s['ei'][s['par'], :, 0].cpu().numpy()))

    eng._iter = _iter
    return eng.run(nm, ini), rec


def test_short_run_against_the_host_contract():
    """arch (2, 8, 1) tanh, 3 chains, adapt = 40, nmcmc = 48, max_depth = 4, to the standard of
    test_gpu_nuts.py::test_short_run_against_the_host_contract: `nuts_iter` (adapt = 0) and `nuts_warm_update` on the host, fed
    the device's momenta and the same operator's SSE and gradients, make the decisions of the device run -- depth and nleap of
    every step are equal and the stored rows, the step sizes and the scales equal BIT FOR BIT.  A seed whose host run has a
    decision within 1e-9 of a tie is passed over, at most 2 of 10.  Host and device advance one leapfrog of every live chain
    per iteration, so the scalars the device formed with its exp / log / pow after iteration n (read behind every `_iter`) are
    handed to the contract's update of iteration n (`given`), as `nuts_iter` takes `eps_next`: what is left is elementwise.
    Each of those scalars is also compared with the contract's own from the same inputs (the device's acceptance statistic of
    the step among them), to 1e-12 relative as tests/test_gpu_hmc_adapt.py compares the same formulas."""
    x, y = _problem(32, 2)
    C, nm, p, adapt = 3, 48, ARCH.nparams, 40
    ini = _ini(C)
    plan = warmup_plan(adapt, True)
    skipped = 0
    for seed in range(10):
        res, rec = _recorded_run(DeviceNUTS(BatchedMLP(ARCH, x, y), 0.2, seed=seed, adapt_mass=True, **HOST_RUN), nm, ini)
        dev_alphas = res['alphas'].cpu().numpy()
        op = BatchedMLP(ARCH, x, y)
        Z = [device_momenta(seed, 0, C, p, t)[0] for t in range(nm)]
        sse0, g0 = (a.cpu().numpy() for a in op.sse_grad(ini))
        cfgs = [nuts.nuts_config(0.2, 32, nm, 4, adapt, 0.8, seed=seed, chain=c) for c in range(C)]
        sts = [nuts.nuts_init(ini[c], sse0[c], g0[c], 0.02, cfgs[c], Z[0][c]) for c in range(C)]
        wss = [na.warm_state(0.02, p) for _ in range(C)]
        rows = {k: np.zeros((C, nm + 1), dtype=np.int64) for k in ('depth', 'nleap')}
        chain, lps, alphas = np.zeros((C, nm + 1, p)), np.zeros((C, nm + 1)), np.zeros((C, nm + 1))
        margin, it, synced, worst = np.inf, 0, True, 0.0
        while min(st['t'] for st in sts) < nm:
            sse, g = (a.cpu().numpy() for a in op.sse_grad(np.stack([st['q'] for st in sts])))
            for c in range(C):
                if sts[c]['t'] >= nm:
                    continue
                t1, old = sts[c]['t'] + 1, sts[c]
                new, _ = nuts.nuts_iter(old, sse[c], g[c], dict(cfgs[c], adapt=0), z_next=Z[t1][c] if t1 < nm else None)
                margin = min(margin, new['margin'])
                if 'row' in new:
                    row, crow, lps[c, row], alphas[c, row], dep, nl = new['row']
                    chain[c, row], rows['depth'][c, row], rows['nleap'][c, row] = crow, dep, nl
                synced = synced and it < len(rec) and rec[it][1][c] == new['t']     # (the device ended the same steps so far)
                given = None
                if synced and new['t'] == t1 <= adapt:
                    given = dict(zip(('mu', 'hbar', 'logbar', 'eps'), rec[it][0][c]))
                    own, wown, _ = na.nuts_warm_update(old, new, wss[c], cfgs[c], plan, dev_alphas[c])
                    for key, a, b in [('eps', given['eps'], own['eps'])] + [(k, given[k], wown[k]) for k in ('mu', 'hbar', 'logbar')]:
                        worst = max(worst, abs(a - b) / abs(b) if b else abs(a))
                sts[c], wss[c], cfgs[c] = na.nuts_warm_update(old, new, wss[c], cfgs[c], plan, alphas[c], given=given)
            it += 1
        if margin < 1e-9:
            skipped += 1
            continue
        dch = np.max(np.abs(res['chain'][:, 1:].cpu().numpy() - chain[:, 1:]), axis=(0, 2))
        print("seed %d: scalars device against contract, worst relative difference %.3g; rows: first differing step %s, largest "
              "difference %.3g" % (seed, worst, (np.nonzero(dch)[0][:1] + 1).tolist(), dch.max()))
        assert synced
        assert np.array_equal(res['depth'].cpu().numpy(), rows['depth']) and np.array_equal(res['nleap'].cpu().numpy(), rows['nleap'])
        assert np.array_equal(res['chain'][:, 1:].cpu().numpy(), chain[:, 1:])
        # energies are sums over N = 32 rows and p = 33 momenta of size ~1: the two summation orders differ by ~1e-14 absolute
        # on dE, so 1e-12 on the acceptance statistic (a mean of min(1, exp(-dE))) and relative on the log-posterior
        assert np.max(np.abs(res['alphas'][:, 1:].cpu().numpy() - alphas[:, 1:])) <= 1e-12
        assert np.max(np.abs(res['logpost'][:, 1:].cpu().numpy() - lps[:, 1:]) / np.abs(lps[:, 1:])) <= 1e-12
        assert worst <= 1e-12
        assert np.array_equal(res['epsilon'].cpu().numpy(), [st['eps'] for st in sts])
        assert np.array_equal(res['mass_scale'].cpu().numpy(), np.stack([cfg['scale'] for cfg in cfgs]))
        assert res['nwarm'] == adapt and not np.array_equal(res['mass_scale'].cpu().numpy(), np.ones((C, p)))
        break
    assert skipped <= 2


RUN = dict(epsilon=0.02, max_depth=4, seed=9, block=8, adapt=40, adapt_mass=True)
AKEYS = KEYS + ('mass_scale',)


@pytest.fixture(scope="module")
def whole_run():
    x, y = _problem(32, 2)
    return DeviceNUTS(BatchedMLP(ARCH, x, y), 0.2, chain0=0, **RUN).run(48, _ini())


def test_chains_do_not_depend_on_how_they_are_split(whole_run):
    """6 chains in one engine, as 2 x 3 engines and as 2 groups: the same bits, `mass_scale` and `epsilon` included; and
    through `NN_MCMC.fit` with sampler_params={'adapt': 40, 'adapt_mass': True}."""
    x, y = _problem(32, 2)
    ini, whole = _ini(), whole_run
    parts = []
    for c0, c1 in ((0, 3), (3, 6)):
        op = BatchedMLP(ARCH, x, y)
        op.set_plan_batch(6)                    # split every chain's rows as the launch of all six chains does
        parts.append(DeviceNUTS(op, 0.2, chain0=c0, **RUN).run(48, ini[c0:c1]))
    for k in AKEYS:
        assert torch.equal(torch.cat([parts[0][k], parts[1][k]]), whole[k]), k
    two = DeviceNUTS(BatchedMLP(ARCH, x, y), 0.2, chain0=0, groups=2, **RUN).run(48, ini)
    for k in AKEYS:
        assert torch.equal(two[k], whole[k]), k
    assert whole['nwarm'] == 40 and whole['mass_scale'].shape == (6, ARCH.nparams)
    assert torch.isfinite(whole['chain']).all() and torch.isfinite(whole['mass_scale']).all() and (whole['mass_scale'] > 0).all()
    assert (whole['mass_scale'] != 1).all() and (whole['epsilon'] != 0.02).all()
    # the step sizes are frozen after warm-up: a longer run of the same chains ends with the same ones
    longer = DeviceNUTS(BatchedMLP(ARCH, x, y), 0.2, chain0=0, **RUN).run(56, ini)
    assert torch.equal(longer['epsilon'], whole['epsilon']) and torch.equal(longer['mass_scale'], whole['mass_scale'])
    assert torch.equal(longer['chain'][:, :49], whole['chain'])
    from quinn_amd.nns.mlp import MLP
    from quinn_amd.solvers.nn_mcmc import NN_MCMC
    uq = NN_MCMC(MLP(2, 1, (8,), activ="tanh"), verbose=False)
    sp = {k: v for k, v in RUN.items() if k != 'seed'}
    uq.fit(x, y, zflag=False, datanoise=0.2, nmcmc=48, param_ini=ini, sampler='nuts', engine='device', seeds=[9] + list(range(5)),
           diagnostics=True, sampler_params=dict(sp, groups=2))
    r = uq.mcmc_results
    for k in AKEYS:
        assert np.array_equal(r[k], whole[k].cpu().numpy()), k
    assert r['nwarm'] == 40 and np.isfinite(uq.diagnostics['logpost']['rhat']).all()


def _counting(monkeypatch):
    L, calls = _lib.lib(), []
    real = L.qn_nuts_adapt
    monkeypatch.setattr(L, 'qn_nuts_adapt', lambda *a: calls.append(1) or real(*a), raising=False)
    return calls


def test_the_default_path_makes_no_new_launch(monkeypatch, whole_run):
    x, y = _problem(32, 2)
    ini = _ini()
    calls = _counting(monkeypatch)
    base = dict(epsilon=0.02, max_depth=4, seed=9, block=8)
    plain = DeviceNUTS(BatchedMLP(ARCH, x, y), 0.2, adapt=12, **base).run(20, ini)
    assert 'mass_scale' not in plain and not calls
    # adapt_mass=True without windows (adapt < 20): the same launches, the same bits; mass_scale is None
    nowin = DeviceNUTS(BatchedMLP(ARCH, x, y), 0.2, adapt=12, adapt_mass=True, **base).run(20, ini)
    assert not calls and nowin['mass_scale'] is None and list(nowin)[:-1] == list(plain)
    for k in KEYS:
        assert torch.equal(nowin[k], plain[k]), k
    # a handed-over scale still works, with and without windows: a scale of ones is the run without one
    ones = DeviceNUTS(BatchedMLP(ARCH, x, y), 0.2, adapt=12, mass_scale=np.ones((6, ARCH.nparams)), **base).run(20, ini)
    for k in KEYS:
        assert torch.equal(ones[k], plain[k]), k
    assert not calls
    mine = torch.ones(6, ARCH.nparams, dtype=torch.float64, device="cuda")
    eng = DeviceNUTS(BatchedMLP(ARCH, x, y), 0.2, mass_scale=mine, **RUN)
    again = eng.run(48, ini)
    assert (mine == 1).all()                                        # the engine adapts a copy, not the caller's tensor
    for k in AKEYS:
        assert torch.equal(again[k], whole_run[k]), k
    # with windows the launch follows every iteration until the host has seen the slowest chain leave the warm-up
    assert 40 <= len(calls) <= eng.last_iters[0]
    given = 0.8 + 0.4 * np.random.RandomState(4).rand(6, ARCH.nparams)
    start = DeviceNUTS(BatchedMLP(ARCH, x, y), 0.2, mass_scale=given, **RUN).run(48, ini)
    assert not torch.equal(start['chain'][:, 1], whole_run['chain'][:, 1]) and torch.isfinite(start['mass_scale']).all()


def test_windows_shorten_the_trajectories_of_an_ill_scaled_exact_target():
    """The linear model of test_ess_contract with its input columns scaled by 1 and 0.01 (dims (2, 1) with bias, N = 32, sigma =
    0.5, priorsigma = 10: the posterior's standard deviations are ~0.15, ~8 and ~0.09), 8 chains from w = 0, adapt = 150, 250
    steps, max_depth = 8.  As on the CPU (tests/test_nuts_adapt_contract.py): the mean nleap after warm-up with unit mass is at
    least 4 times that with windows.  The windowed run's post-warm-up means and second central moments against
    `gaussian_posterior`, each within 5 standard errors from the batch-means ESS of that quantity's trace -- the yardstick of
    test_gpu_nuts.py::test_exact_target_linear_model."""
    x, y = linear_problem()
    x = x * np.array([1.0, 0.01])
    s = 10.0
    op = BatchedMLP(MLPArch((2, 1), "identity"), x, y[:, None])
    X = np.hstack([x, np.ones((LIN_N, 1))])
    g = op.sse_grad(np.zeros((1, 3)))[1][0].double().cpu().numpy()
    want_g = -2.0 * X.T @ y
    perm = [int(np.argmin(np.abs(want_g - gi))) for gi in g]
    assert sorted(perm) == [0, 1, 2]
    mean, cov = gaussian_posterior(X[:, perm], y, LIN_SIGMA, s)
    kw = dict(epsilon=0.05, max_depth=8, adapt=150, priorsigma=s, seed=1)
    unit = DeviceNUTS(op, LIN_SIGMA, **kw).run(250, np.zeros((8, 3)))
    wind = DeviceNUTS(op, LIN_SIGMA, adapt_mass=True, **kw).run(250, np.zeros((8, 3)))
    nl_unit, nl_wind = float(unit['nleap'][:, 151:].double().mean()), float(wind['nleap'][:, 151:].double().mean())
    ch = wind['chain'][:, 151:]
    d = ch - torch.as_tensor(mean, device=ch.device)
    iu = np.triu_indices(3)
    traces = torch.cat([ch, (d[:, :, :, None] * d[:, :, None, :])[:, :, iu[0], iu[1]]], dim=2).contiguous()
    st = diag.diagnose_chains(traces, 0)
    err = np.abs(st['mean'] - np.concatenate([mean, cov[iu]])) / np.sqrt(st['var'] / st['ess'])
    print("mean nleap after warm-up: unit mass %.1f, with windows %.1f; eps %.3g / %.3g; scale %s against sd %s; standard errors: "
          "mean %.2f, covariance %.2f; ndiv %d" % (nl_unit, nl_wind, float(unit['epsilon'].mean()), float(wind['epsilon'].mean()),
                                                  wind['mass_scale'].mean(dim=0).cpu().numpy(), np.sqrt(np.diag(cov)), err[:3].max(),
                                                  err[3:].max(), int(wind['ndiv'].sum())))
    assert nl_unit >= 4 * nl_wind
    assert err[:3].max() <= 5.0 and err[3:].max() <= 5.0


def test_refusals():
    L = _lib.lib()
    for over in REFUSED:
        assert L.qn_nuts_adapt(*adapt_abi_args(**over)) == _lib.CONSTANTS["QN_EINVAL"], over
        assert b"qn_nuts_adapt" in L.qn_last_error(), over
    x, y = _problem(16, 2)
    op = BatchedMLP(ARCH, x, y)
    with pytest.raises(ValueError, match="adapt_mass"):
        DeviceNUTS(op, 0.2, adapt_mass=True)
    with pytest.raises(ValueError, match="adapt_mass"):
        DeviceNUTS(op, 0.2, adapt=40, adapt_mass=1)
    with pytest.raises(ValueError, match="use_graph"):
        DeviceNUTS(op, 0.2, adapt=40, adapt_mass=True, use_graph=True)
    with pytest.raises(ValueError, match="ladder"):
        DeviceNUTS(op, 0.2, adapt=40, adapt_mass=True, ladder=4)
    with pytest.raises(ValueError, match="adapt"):
        DeviceNUTS(op, 0.2, adapt=40, adapt_mass=True).run(20, _ini())
    from quinn_amd.nns.mlp import MLP
    from quinn_amd.solvers.nn_mcmc import NN_MCMC
    uq = NN_MCMC(MLP(2, 1, (8,), activ="tanh"), verbose=False)
    with pytest.raises(ValueError, match="adapt_mass"):
        uq.fit(x, y, zflag=False, nmcmc=48, param_ini=np.zeros(uq.pdim), sampler='nuts', engine='device',
               sampler_params={'adapt_mass': True})
