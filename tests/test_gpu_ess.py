"""GPU: elliptical slice sampling on the device (qn_ess_begin / qn_ess_iter, `DeviceESS`, `NN_MCMC.fit(sampler='ess')`).  One
iteration with every branch in one launch is compared with the numpy restatement, the random streams with their keys, the
chains for independence from the way they are split, the bookkeeping with the solver's log-posterior, and the sampler in
distribution with the closed-form posterior of a linear model."""
import numpy as np
import pytest
import torch

from quinn_amd import _lib
from quinn_amd.mcmc import ess
from quinn_amd.mcmc.device_ess import DeviceESS
from quinn_amd.ops import BatchedMLP, MLPArch

from test_ess_contract import N as LIN_N, S as LIN_S, SIGMA as LIN_SIGMA, ess_abi_cases, linear_problem

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
KEYS = ('chain', 'logpost', 'alphas', 'accrate', 'mapparams', 'maxpost', 'nev', 'ntrunc', 'nevals')


class Raw:
    """The two entry points through the C ABI on tensors of its own."""

    def __init__(self, C, p, nmcmc, chain0, seed, sigma=0.5, s=0.8, n_rows=20, max_shrink=4, f32=False, data_seed=0):
        dev, f64 = "cuda", torch.float64
        rs = np.random.RandomState(data_seed)
        self.C, self.p, self.nmcmc, self.chain0, self.seed = C, p, nmcmc, chain0, seed
        self.sigma, self.s, self.n_rows, self.max_shrink = sigma, s, n_rows, max_shrink
        self.nwg = int(_lib.lib().qn_hmc_parts(p))
        t = lambda a: torch.as_tensor(a, dtype=f64, device=dev)
        self.cur, self.sse_cur, self.lp_cur = t(rs.randn(C, p)), t(rs.rand(C) * 5 + 1), t(-rs.rand(C) * 30)
        self.nu, self.prop = t(np.full((C, p), np.nan)), t(np.full((C, p), np.nan))
        self.prop_op = torch.full((C, p), np.nan, dtype=torch.float32, device=dev) if f32 else None
        self.qdt = _lib.QN_F32 if f32 else _lib.QN_F64
        self.sq = t(np.full((2, C, self.nwg), np.nan))
        self.es = t(np.full((2, C, 6), np.nan))
        self.ei = torch.full((2, C, 4), -7, dtype=torch.int64, device=dev)
        self.best, self.best_lp = t(np.full((C, p), 99.0)), t(np.full((2, C), np.nan))
        self.chain, self.lps = t(np.full((C, nmcmc + 1, p), np.nan)), t(np.full((C, nmcmc + 1), np.nan))
        self.nev = torch.full((C, nmcmc + 1), -1, dtype=torch.int32, device=dev)

    def begin(self):
        ptr = lambda a: None if a is None else a.data_ptr()
        _lib.check(_lib.lib().qn_ess_begin(self.cur.data_ptr(), self.sse_cur.data_ptr(), self.lp_cur.data_ptr(), self.sigma, self.s,
                                           self.C, self.chain0, self.p, self.seed, self.nu.data_ptr(), self.prop.data_ptr(),
                                           ptr(self.prop_op), self.qdt, self.sq.data_ptr(), self.es.data_ptr(),
                                           self.ei.data_ptr(), None), "qn_ess_begin")
        torch.cuda.synchronize()

    def iter(self, sse_prop, parity):
        ptr = lambda a: None if a is None else a.data_ptr()
        _lib.check(_lib.lib().qn_ess_iter(
            sse_prop.data_ptr(), sse_prop.shape[1], self.sigma, self.s, self.n_rows, self.max_shrink, self.C, self.chain0, self.p,
            self.nmcmc, self.seed, self.cur.data_ptr(), self.nu.data_ptr(), self.prop.data_ptr(), ptr(self.prop_op), self.qdt,
            self.best.data_ptr(), self.best_lp.data_ptr(), self.chain.data_ptr(), self.lps.data_ptr(), self.nev.data_ptr(),
            self.sq.data_ptr(), self.es.data_ptr(), self.ei.data_ptr(), parity, None), "qn_ess_iter")
        torch.cuda.synchronize()

    def host(self):
        return {k: getattr(self, k).cpu().numpy().copy() for k in ('cur', 'nu', 'prop', 'sq', 'es', 'ei', 'best', 'best_lp', 'chain',
                                                                    'lps', 'nev')}


def _close_prop(got, cur, nu, theta):
    """prop against numpy's ellipse: the device sincos and numpy's differ by a few ulp each."""
    return np.all(np.abs(got - ess.ellipse(cur, nu, theta)) <= 8 * U * (np.abs(cur) + np.abs(nu)))


@pytest.mark.parametrize("p", [13, 1153])
@pytest.mark.parametrize("nparts", [1, 3])
def test_one_iteration_every_branch_against_numpy(p, nparts):
    """C = 5, chain0 = 7, one launch: chain 0 accepts (and starts its next step), 1 shrinks from the left, 2 shrinks from the
    right (on a NaN SSE), 3 is at its last proposal and is truncated, 4 is done.  p = 13: odd, one workgroup; p = 1153: two."""
    C, chain0, seed, nmcmc, ms = 5, 7, 11, 6, 4
    r = Raw(C, p, nmcmc, chain0, seed, max_shrink=ms, f32=True)
    gs = -0.5 / r.sigma ** 2
    r.begin()
    h0 = r.host()
    assert r.nwg == (1 if p == 13 else 2)
    # ---- qn_ess_begin itself: step 0 of every chain
    ut, uy = ess.start_uniforms(seed, 0, chain0 + np.arange(C))
    for c in range(C):
        b = ess.ess_begin(h0['cur'][c], float(r.sse_cur[c]), h0['nu'][c], ut[c], uy[c], r.sigma)
        assert [b['theta'], b['tmin'], b['tmax'], b['logy']] == list(h0['es'][0, c, :4]), c
        assert h0['es'][0, c, 4] == float(r.sse_cur[c]) and h0['es'][0, c, 5] == float(r.lp_cur[c])
        assert _close_prop(h0['prop'][c], h0['cur'][c], h0['nu'][c], b['theta'])
        assert abs(h0['sq'][0, c].sum() - np.sum(h0['prop'][c] ** 2)) <= 1e-13 * np.sum(h0['prop'][c] ** 2)
    assert np.array_equal(h0['ei'][0], np.zeros((C, 4), dtype=np.int64))
    assert torch.equal(r.prop_op, r.prop.float())
    # ---- the five states of the launch, written into slot 0
    ei, es = h0['ei'][0].copy(), h0['es'][0].copy()
    ei[0] = (2, 1, 0, 9)                                            # accepts at its second proposal of step 2
    ei[1] = (1, 1, 1, 5)
    es[1, 0] = 0.5 * es[1, 1]                                       # theta < 0: the bracket shrinks from the left
    ei[2] = (0, 0, 0, 0)                                            # theta > 0 as begun: from the right
    ei[3] = (3, ms - 1, 2, 17)                                      # at its last proposal
    ei[4] = (nmcmc, 0, 1, 23)                                       # done
    r.ei[0] = torch.as_tensor(ei, device="cuda")
    r.es[0] = torch.as_tensor(es, device="cuda")
    blp = np.array([-np.inf, 1.0, 2.0, 3.0, 4.0])                   # chain 0's new point is its best
    r.best_lp[0] = torch.as_tensor(blp, device="cuda")
    sse = np.array([0.5 * es[0, 3] / gs, 1e9, np.nan, 1e9, 0.25])   # gs sse > logy for chain 0 only
    rs = np.random.RandomState(3)
    parts = rs.rand(C, nparts) + 0.5
    parts *= (sse / parts.sum(axis=1))[:, None]
    tot = parts[:, 0].copy()
    for k in range(1, nparts):
        tot = tot + parts[:, k]                                     # left to right, as the kernel adds them
    r.iter(torch.as_tensor(parts, dtype=torch.float64, device="cuda"), 0)
    h1 = r.host()
    # ---- numpy, fed the device's own nu of chain 0's next step
    events = []
    for c in range(C):
        st = {'cur': h0['cur'][c], 'nu': h0['nu'][c], 'prop': h0['prop'][c], 'best': h0['best'][c], 'best_lp': blp[c]}
        st.update(zip(ess.ES_KEYS, es[c]))
        st.update(zip(ess.EI_KEYS, (int(v) for v in ei[c])))
        t, j = st['t'], st['j']
        un = ess.start_uniforms(seed, t + 1, chain0 + c)
        want, event = ess.ess_iter(st, tot[c], r.sigma, r.s, r.n_rows, nmcmc, ms, u_shrink=ess.shrink_uniform(seed, t, chain0 + c, j + 1),
                                   nu_next=h1['nu'][c], u_next=un, sq_prop=(h0['sq'][0, c, 0] if r.nwg == 1 else
                                                                            h0['sq'][0, c, 0] + h0['sq'][0, c, 1]))
        events.append(event)
        got_es, got_ei = h1['es'][1, c], h1['ei'][1, c]
        assert [want[k] for k in ess.EI_KEYS] == list(got_ei), (c, event)
        assert [want[k] for k in ess.ES_KEYS[:5]] == list(got_es[:5]), (c, event)              # bit for bit
        assert abs(want['lp_cur'] - got_es[5]) <= 1e-12 * abs(want['lp_cur']), (c, event)
        assert np.array_equal(want['cur'], h1['cur'][c]), (c, event)
        if event == 'done':
            continue
        assert _close_prop(h1['prop'][c], want['cur'], want['nu'], want['theta']), (c, event)
        assert abs(h1['sq'][1, c].sum() - np.sum(h1['prop'][c] ** 2)) <= 1e-13 * np.sum(h1['prop'][c] ** 2)
        rows = np.isfinite(h1['lps'][c])
        if event == 'shrink':
            assert not rows.any() and np.array_equal(h1['nu'][c], h0['nu'][c]) and h1['best_lp'][1, c] == blp[c]
            assert np.array_equal(h1['best'][c], h0['best'][c]) and (h1['nev'][c] == -1).all()
            continue
        row, crow, lp, ne = want['row']
        assert list(np.flatnonzero(rows)) == [row] and row == t + 1
        assert np.array_equal(h1['chain'][c, row], crow) and h1['nev'][c, row] == ne and (np.delete(h1['nev'][c], row) == -1).all()
        assert np.isnan(np.delete(h1['chain'][c], row, axis=0)).all()
        assert abs(h1['lps'][c, row] - lp) <= 1e-12 * abs(lp) and h1['lps'][c, row] == got_es[5]
        assert not np.array_equal(h1['nu'][c], h0['nu'][c])                                     # a new partner was drawn
        if event == 'accept':
            assert np.array_equal(h1['best'][c], h0['prop'][c]) and h1['best_lp'][1, c] == got_es[5]
        else:
            assert np.array_equal(h1['best'][c], h0['best'][c]) and h1['best_lp'][1, c] == blp[c]
    assert events == ['accept', 'shrink', 'shrink', 'trunc', 'done']
    assert h1['ei'][1, 1, 1] == 2 and h1['es'][1, 1, 1] == es[1, 0] and h1['es'][1, 1, 2] == es[1, 2]   # from the left: tmin moved
    assert h1['ei'][1, 2, 1] == 1 and h1['es'][1, 2, 2] == es[2, 0] and h1['es'][1, 2, 1] == es[2, 1]   # from the right: tmax moved
    # ---- the done chain: nothing but the copy of its scalars
    for k in ('cur', 'nu', 'prop', 'best', 'chain', 'lps', 'nev'):
        assert np.array_equal(h1[k][4], h0[k][4], equal_nan=True), k
    assert np.array_equal(h1['es'][1, 4], es[4]) and np.array_equal(h1['ei'][1, 4], ei[4]) and h1['best_lp'][1, 4] == blp[4]
    assert np.array_equal(h1['sq'][1, 4], h0['sq'][0, 4])
    # ---- slot 0 was only read; the float32 operator's copy is the proposal rounded once
    assert np.array_equal(h1['es'][0], es, equal_nan=True) and np.array_equal(h1['ei'][0], ei)
    assert torch.equal(r.prop_op, r.prop.float())


def test_normals_and_uniforms_are_keyed_by_seed_step_and_global_chain():
    C, p, s = 4, 8192, 0.8
    def nu_of(seed, chain0, t):
        """The partner of step t: begun at step 0 (t = 0), or drawn by an accepting iteration of step t - 1."""
        r = Raw(C, p, 9, chain0, seed, s=s)
        r.begin()
        if t > 0:
            r.ei[0, :, 0] = t - 1
            r.iter(torch.zeros(C, 1, dtype=torch.float64, device="cuda"), 0)        # SSE 0: gs sse = 0 > logy, every chain accepts
            assert (r.ei[1, :, 0] == t).all()
        return r.nu.cpu().numpy(), r.es[1 if t > 0 else 0].cpu().numpy()
    a, es_a = nu_of(5, 10, 0)
    z = a / s
    n = z.size
    assert abs(z.mean()) <= 5 / np.sqrt(n) and abs(z.var() - 1.0) <= 5 / np.sqrt(n)
    assert np.array_equal(a, nu_of(5, 10, 0)[0])
    b, es_b = nu_of(5, 12, 0)                                       # global chains 12 .. 15: two of them are a's
    assert np.array_equal(b[:2], a[2:]) and np.array_equal(es_b[:2, :3], es_a[2:, :3])     # (logy also holds the chain's SSE)
    for other in ((6, 10, 0), (5, 10, 3), (5, 14, 0)):
        o, _ = nu_of(*other)
        assert not np.any(o == a), other
    # the angle uniforms are sgmcmc.philox4x32's, bit for bit, at step 0 and at step 3
    _, es3 = nu_of(5, 10, 3)
    for t, es_t in ((0, es_a), (3, es3)):
        ut, _ = ess.start_uniforms(5, t, 10 + np.arange(C))
        assert np.array_equal(es_t[:, 0], 2.0 * np.pi * ut), t


def _problem(N, d, seed=0):
    rs = np.random.RandomState(seed)
    x = rs.rand(N, d) * 4 - 2
    y = np.sin(x).sum(axis=1, keepdims=True) + 0.1 * rs.randn(N, 1)
    return x, y


def test_chains_do_not_depend_on_how_they_are_split():
    x, y = _problem(64, 2)
    arch = MLPArch((2, 3, 1), "tanh")
    ini = np.stack([np.random.RandomState(50 + c).rand(arch.nparams) for c in range(6)])
    kw = dict(priorsigma=1.5, seed=9, block=16)
    whole = DeviceESS(BatchedMLP(arch, x, y), 0.2, chain0=0, **kw).run(200, ini)
    parts = []
    for c0, c1 in ((0, 2), (2, 6)):
        op = BatchedMLP(arch, x, y)
        op.set_plan_batch(6)                    # split every chain's rows as the launch of all six chains does
        parts.append(DeviceESS(op, 0.2, chain0=c0, **kw).run(200, ini[c0:c1]))
    for k in KEYS:
        assert torch.equal(torch.cat([parts[0][k], parts[1][k]]), whole[k]), k
    two = DeviceESS(BatchedMLP(arch, x, y), 0.2, chain0=0, groups=2, **kw).run(200, ini)
    for k in KEYS:
        assert torch.equal(two[k], whole[k]), k
    assert torch.isfinite(whole['chain']).all() and (whole['nev'][:, 1:] >= 1).all()


def test_bookkeeping_against_the_solver_log_posterior():
    from quinn_amd.nns.mlp import MLP
    from quinn_amd.solvers.nn_mcmc import NN_MCMC
    x, y = _problem(32, 1)
    uq = NN_MCMC(MLP(1, 1, (5,), activ="tanh"), verbose=False)
    ini = np.stack([np.random.RandomState(c).rand(uq.pdim) for c in range(3)])
    uq.fit(x, y, zflag=False, datanoise=0.2, nmcmc=150, param_ini=ini, sampler='ess', engine='device', priorsigma=1.2,
           seeds=[3, 4, 5], sampler_params={})
    r = uq.mcmc_results
    C, T, p = r['chain'].shape
    assert (C, T, p) == (3, 151, uq.pdim) and r['nev'].shape == (3, 151) and r['nev'].dtype == np.int32
    want = uq.logpost_batch(r['chain'].reshape(C * T, p)).reshape(C, T)
    assert np.max(np.abs(r['logpost'] - want) / np.abs(want)) <= 1e-10
    assert np.array_equal(r['maxpost'], r['logpost'].max(axis=1))
    for c in range(C):
        assert np.array_equal(r['mapparams'][c], r['chain'][c, int(r['logpost'][c].argmax())])
    assert np.array_equal(r['nev'].sum(axis=1), r['nevals']) and (r['nev'][:, 0] == 0).all() and (r['nev'][:, 1:] >= 1).all()
    assert (r['ntrunc'] == 0).all() and (r['accrate'] == 1.0).all() and (r['alphas'] == 1.0).all()
    assert (r['chain'][:, 1:] != r['chain'][:, :-1]).any(axis=2).all()          # every step moves


def test_exact_target_linear_model():
    """dims = (2, 1) with bias, N = 32, sigma = 0.5, s = 1, 16 chains x 2000 steps from w = 0, the first tenth dropped, against
    `gaussian_posterior`.  The bar comes from the numpy restatement at the same counts (tests/test_ess_contract.py,
    run_restatement(seed, 16, 2000, 32) for the seeds 1 .. 5): dm = 0.0094, 0.0277, 0.0286, 0.0216, 0.0114 and dc = 0.0143,
    0.0131, 0.0351, 0.0192, 0.0193, no truncated step; 3 x the largest of each is 0.0858 and 0.1053."""
    x, y = linear_problem()
    arch = MLPArch((2, 1), "identity")
    op = BatchedMLP(arch, x, y[:, None])
    # the flat weight vector in the design matrix's terms: d sse / d w at w = 0 tells which entry multiplies which column
    X = np.hstack([x, np.ones((LIN_N, 1))])
    g = op.sse_grad(np.zeros((1, 3)))[1][0].double().cpu().numpy()
    want_g = -2.0 * X.T @ y
    perm = [int(np.argmin(np.abs(want_g - gi))) for gi in g]
    assert sorted(perm) == [0, 1, 2] and np.allclose(g, want_g[perm], rtol=1e-9)
    mean, cov = ess.gaussian_posterior(X[:, perm], y, LIN_SIGMA, LIN_S)
    res = DeviceESS(op, LIN_SIGMA, priorsigma=LIN_S, seed=1).run(2000, np.zeros((16, 3)))
    assert (res['ntrunc'] == 0).all()
    dm, dc = ess.moment_deviation(res['chain'][:, 200:].reshape(-1, 3).cpu().numpy(), mean, cov)
    print("dm = %.4f dc = %.4f mean nev = %.2f" % (dm, dc, float(res['nev'][:, 1:].double().mean())))
    assert dm <= 3 * 0.0286 and dc <= 3 * 0.0351


def test_float32_operator_reads_the_proposal_rounded_once():
    x, y = _problem(48, 1)
    arch = MLPArch((1, 8, 1), "tanh")
    ini = np.stack([np.random.RandomState(c).rand(arch.nparams) for c in range(3)])
    op = BatchedMLP(arch, x, y, dtype="float32")
    seen = []
    fwd = op.sse_parts
    def spy(W):
        seen.append(W)
        return fwd(W)
    op.sse_parts = spy
    eng = DeviceESS(op, 0.2, priorsigma=1.0, seed=2, block=4)
    res = eng.run(20, ini)
    assert seen and all(W.dtype == torch.float32 for W in seen)
    assert torch.isfinite(res['logpost']).all() and (res['nev'][:, 1:] >= 1).all()
    # the engine's float32 buffer is the float64 proposal rounded once (every launch writes both; the branch test above checks
    # the kernels' every branch): Raw with f32 after a begin and an all-accepting iteration
    r = Raw(3, 37, 5, 0, 4, f32=True)
    r.begin()
    assert torch.equal(r.prop_op, r.prop.float())
    r.iter(torch.zeros(3, 1, dtype=torch.float64, device="cuda"), 0)
    assert torch.equal(r.prop_op, r.prop.float()) and (r.ei[1, :, 0] == 1).all()


def test_through_the_solver():
    from quinn_amd.nns.mlp import MLP
    from quinn_amd.solvers.nn_mcmc import NN_MCMC
    x, y = _problem(64, 1)
    uq = NN_MCMC(MLP(1, 1, (16, 16), activ="tanh"), verbose=False)
    ini = np.stack([np.random.RandomState(c).rand(uq.pdim) for c in range(4)])
    uq.fit(x, y, zflag=False, datanoise=0.2, nmcmc=120, param_ini=ini, sampler='ess', engine='device', priorsigma=1.0,
           seeds=range(4), diagnostics=True, sampler_params={'max_shrink': 32, 'block': 16})
    r = uq.mcmc_results
    assert uq.lpinfo['lparams']['priorsigma'] == 1.0
    assert set(KEYS) <= set(r) and r['chain'].shape == (4, 121, uq.pdim) and r['logpost'].shape == (4, 121)
    assert r['nev'].shape == (4, 121) and r['ntrunc'].shape == (4,) and r['nevals'].shape == (4,) and r['accrate'].shape == (4,)
    for k in KEYS:
        assert np.isfinite(np.asarray(r[k], dtype=np.float64)).all(), k
    d = uq.diagnostics
    assert set(d) == {'params', 'logpost'} and np.isfinite(d['logpost']['rhat']).all() and np.isfinite(d['params']['ess']).all()
    pred = uq.predict_ens(x, nens=8, nburn=60, chain='all')
    assert pred.shape == (8, 64, 1) and np.isfinite(pred).all()
    sc = uq.score(x, y, nsam=8, nburn=60, chain='all')
    assert all(np.isfinite(sc[k]) for k in ('lppd', 'nlpd', 'crps', 'rmse', 'waic')) and np.isfinite(sc['pit']).all()
    assert np.isfinite(uq.diagnose(nburn=60)['params']['rhat']).all()


def test_argument_refusals_of_both_entry_points():
    L = _lib.lib()
    for name, ok, bads in ess_abi_cases():
        for bad in bads:
            assert getattr(L, name)(*dict(ok, **bad).values()) == _lib.CONSTANTS["QN_EINVAL"], (name, bad)
            assert name.encode() in L.qn_last_error(), (name, bad)
