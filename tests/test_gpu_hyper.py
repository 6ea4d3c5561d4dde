"""GPU: the hierarchical weight prior of the device HMC / MALA engines.  qn_prior_fold_g against `hyper.fold_g` (gradient bit
for bit, SSE to 1e-13), against qn_prior_fold at equal precisions, alone and among other chains, with non-finite rows;
qn_hyper_gibbs against `hyper.gibbs_round` at both parities with every slot it must not touch checked, and its refusals; the
sampler against the exact moments of the model on a flat likelihood; and the path through `NN_MCMC.fit`."""
import numpy as np
import pytest
import torch

from quinn_amd import _lib
from quinn_amd.mcmc import hyper as hy
from quinn_amd.mcmc.device_hmc import DeviceHMC

pytestmark = pytest.mark.gpu

# (C, p, seg): a one-element group and odd boundaries; boundaries that straddle a workgroup's chunk of a 2500-element row
SHAPES = {"p37": (3, 37, [0, 5, 6, 30, 37]), "p2500": (2, 2500, [0, 1023, 1025, 2500])}
SIGMA, A0, B0 = 0.3, 2.0, 1.5


def _dev(a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def _ptr(t):
    return None if t is None else t.data_ptr()


def _fold_g(W, lam, c0, seg, grad=None, sse=None, stride=1):
    """qn_prior_fold_g through the C ABI on copies of grad / sse -> (grad', sse') numpy, None for None."""
    Wt, lt, ct, st_ = _dev(W), _dev(lam), _dev(c0), _dev(np.asarray(seg, dtype=np.int64))
    gt, st = _dev(grad), _dev(sse)
    gdt = _lib.QN_F32 if gt is not None and gt.dtype == torch.float32 else _lib.QN_F64
    C, p = Wt.shape
    _lib.check(_lib.lib().qn_prior_fold_g(Wt.data_ptr(), lt.data_ptr(), ct.data_ptr(), st_.data_ptr(), len(seg) - 1, _ptr(gt),
                                          gdt, _ptr(st), stride, C, p, None), "qn_prior_fold_g")
    torch.cuda.synchronize()
    assert np.array_equal(Wt.cpu().numpy(), W, equal_nan=True) and np.array_equal(lt.cpu().numpy(), lam)
    return (None if gt is None else gt.cpu().numpy()), (None if st is None else st.cpu().numpy())


def _fold_inputs(name):
    C, p, seg = SHAPES[name]
    rs = np.random.RandomState(p)
    return (C, p, seg, rs.randn(C, p), 3.0 * rs.randn(C, p), 10.0 + 40.0 * rs.rand(C), 10.0 + 40.0 * rs.rand(C, 3),
            0.2 + rs.rand(C, len(seg) - 1), rs.randn(C))


@pytest.mark.parametrize("name", list(SHAPES))
def test_fold_g_equals_the_numpy_fold(name):
    C, p, seg, W, g64, sse1, sse3, lam, c0 = _fold_inputs(name)
    for g in (g64, g64.astype(np.float32)):
        want_g, want_s = hy.fold_g(W, lam, c0, seg, grad=g, sse=sse1)
        got_g, none = _fold_g(W, lam, c0, seg, grad=g)                       # sse NULL
        assert none is None and got_g.dtype == g.dtype
        assert np.array_equal(got_g, want_g)                                 # the same two roundings: bit for bit
        got_g2, got_s = _fold_g(W, lam, c0, seg, grad=g, sse=sse1)
        assert np.array_equal(got_g2, want_g)
        print(name, g.dtype, "sse rel err", np.abs(got_s - want_s) / np.abs(want_s))
        assert np.all(np.abs(got_s - want_s) <= 1e-13 * np.abs(want_s))
        assert np.array_equal(_fold_g(W, lam, c0, seg, sse=sse1)[1], got_s)  # grad NULL: the same sum, another grid
        again = _fold_g(W, lam, c0, seg, grad=g, sse=sse1)
        assert np.array_equal(again[0], got_g2) and np.array_equal(again[1], got_s)
    # sse_stride = 3: column 0 receives the term, the other columns are unchanged bit for bit
    got3 = _fold_g(W, lam, c0, seg, sse=sse3, stride=3)[1]
    assert np.array_equal(got3[:, 1:], sse3[:, 1:])
    want3 = hy.fold_g(W, lam, c0, seg, sse=sse3[:, 0])[1]
    assert np.all(np.abs(got3[:, 0] - want3) <= 1e-13 * np.abs(want3))
    assert np.array_equal(got3[:, 0], _fold_g(W, lam, c0, seg, sse=np.ascontiguousarray(sse3[:, 0]))[1])


@pytest.mark.parametrize("name", list(SHAPES))
def test_fold_g_with_equal_precisions_is_the_scalar_fold_bit_for_bit(name):
    C, p, seg, W, g64, sse1, _, lam, c0 = _fold_inputs(name)
    L = _lib.lib()
    for g in (g64, g64.astype(np.float32)):
        for c in range(C):
            lam_c = float(lam[c, 0])
            got = _fold_g(W[c:c + 1], np.full((1, len(seg) - 1), lam_c), c0[c:c + 1], seg, grad=g[c:c + 1])[0]
            Wt, gt = _dev(W[c:c + 1]), _dev(g[c:c + 1])
            gdt = _lib.QN_F32 if gt.dtype == torch.float32 else _lib.QN_F64
            _lib.check(L.qn_prior_fold(Wt.data_ptr(), lam_c, 0.0, gt.data_ptr(), gdt, None, 1, 1, p, None), "qn_prior_fold")
            torch.cuda.synchronize()
            assert np.array_equal(got, gt.cpu().numpy())


@pytest.mark.parametrize("name", list(SHAPES))
def test_fold_g_a_chain_alone_is_the_chain_among_others_and_non_finite_rows_stay_home(name):
    C, p, seg, W, g64, sse1, _, lam, c0 = _fold_inputs(name)
    for g in (g64, g64.astype(np.float32)):
        whole = _fold_g(W, lam, c0, seg, grad=g, sse=sse1)
        for c in range(C):
            one = _fold_g(W[c:c + 1], lam[c:c + 1], c0[c:c + 1], seg, grad=g[c:c + 1], sse=sse1[c:c + 1])
            assert np.array_equal(one[0][0], whole[0][c]) and one[1][0] == whole[1][c]
    clean_g, clean_s = _fold_g(W, lam, c0, seg, grad=g64, sse=sse1)
    others = [c for c in range(C) if c != 1]
    for bad, check in ((np.inf, lambda v: v == np.inf), (np.nan, np.isnan)):
        Wb = W.copy()
        Wb[1, seg[1]] = bad
        got_g, got_s = _fold_g(Wb, lam, c0, seg, grad=g64, sse=sse1)
        assert check(got_s[1]), (bad, got_s)
        assert np.array_equal(got_s[others], clean_s[others]) and np.array_equal(got_g[others], clean_g[others])
        mask = np.arange(p) != seg[1]
        assert np.array_equal(got_g[1, mask], clean_g[1, mask])


# ------------------------------------------------------------------------------------------------ the Gibbs round
CHAIN0, SEED, STEP, NMCMC, NROUNDS, ROUND = 5, 77, 6, 9, 4, 2


def _gibbs_state(name, seed=0):
    C, p, seg = SHAPES[name]
    rs = np.random.RandomState(1000 + p + seed)
    seg = np.asarray(seg, dtype=np.int64)
    G = len(seg) - 1
    cur = rs.randn(C, p)
    tau = 0.5 + rs.rand(C, G)
    lam, c0 = hy.fold_constants_g(SIGMA, tau, seg, A0, B0)
    gcur, sse = hy.fold_g(cur, lam, c0, seg, grad=3.0 * rs.randn(C, p), sse=10.0 + 40.0 * rs.rand(C))
    taus = rs.rand(C, NROUNDS + 1, G)
    taus[:, ROUND] = tau
    return dict(C=C, p=p, G=G, seg=seg, cur=cur, gcur=gcur, lam=lam, c0=c0, cur_lp=-0.5 * sse / SIGMA ** 2 - 7.0,
                best_lp=rs.randn(C), lps=rs.randn(C, NMCMC + 1), taus=taus)


def _gibbs(st, par, hpar, rows=None, taus=True):
    """qn_hyper_gibbs on device copies of the state (chains `rows`), slot par / hpar current, the other slots filled with
    sentinels -> dict of numpy arrays after the launch."""
    rows = np.arange(st['C']) if rows is None else np.asarray(rows)
    C, G, p = len(rows), st['G'], st['p']

    def two(cur, sentinel, slot):
        a = np.full((2,) + cur.shape, sentinel, dtype=np.float64)
        a[slot] = cur
        return a
    t = {'cur': _dev(st['cur'][rows]), 'gcur': _dev(st['gcur'][rows]), 'cur_lp': _dev(two(st['cur_lp'][rows], -1.5, par)),
         'best_lp': _dev(two(st['best_lp'][rows], -2.5, par)), 'lps': _dev(st['lps'][rows]),
         'lam': _dev(two(st['lam'][rows], -3.5, hpar)), 'c0': _dev(two(st['c0'][rows], -4.5, hpar)), 'seg': _dev(st['seg']),
         'taus': _dev(st['taus'][rows]) if taus else None}
    step = np.full(2, -9, dtype=np.int64)
    step[par] = STEP
    t['step'] = _dev(step)
    rc = _lib.lib().qn_hyper_gibbs(t['cur'].data_ptr(), t['gcur'].data_ptr(), t['cur_lp'].data_ptr(), t['best_lp'].data_ptr(),
                                   t['lps'].data_ptr(), t['lam'].data_ptr(), t['c0'].data_ptr(), t['seg'].data_ptr(),
                                   _ptr(t['taus']), t['step'].data_ptr(), SIGMA, A0, B0, G, ROUND, NROUNDS, C,
                                   CHAIN0 + int(rows[0]), p, NMCMC, SEED, par, hpar, None)
    _lib.check(rc, "qn_hyper_gibbs")
    torch.cuda.synchronize()
    return {k: (None if v is None else v.cpu().numpy()) for k, v in t.items()}


def _close(got, want, rtol, what):
    err = np.abs(got - want).max() / np.abs(want).max()
    print(what, "rel err", err)
    assert err <= rtol, (what, err)


@pytest.mark.parametrize("name", list(SHAPES))
@pytest.mark.parametrize("par,hpar", [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_gibbs_round_equals_the_numpy_round(name, par, hpar):
    st = _gibbs_state(name)
    C = st['C']
    want = hy.gibbs_round(st['cur'], st['gcur'], st['cur_lp'], st['lam'], st['c0'], st['seg'], SIGMA, A0, B0, SEED, STEP, CHAIN0)
    assert want['ok'].all()
    got = _gibbs(st, par, hpar)
    # the new slots
    np.testing.assert_allclose(got['lam'][1 - hpar], want['lam'], rtol=1e-10)
    np.testing.assert_allclose(got['c0'][1 - hpar], want['c0'], rtol=1e-10)
    np.testing.assert_allclose(got['taus'][:, ROUND + 1], want['tau'], rtol=1e-10)
    _close(got['gcur'], want['grad_cur'], 1e-12, "grad_cur")
    _close(got['cur_lp'][1 - par], want['cur_lp'], 1e-12, "cur_lp")
    _close(got['lps'][:, STEP], want['cur_lp'], 1e-12, "lps[:, t]")
    assert np.array_equal(got['lps'][:, STEP], got['cur_lp'][1 - par])
    assert np.array_equal(got['best_lp'][1 - par], st['best_lp']) and got['step'][1 - par] == STEP
    # what the launch reads stays: slot `par` / `hpar` of every double-buffered array, the state, every other stored entry
    assert np.array_equal(got['cur_lp'][par], st['cur_lp']) and np.array_equal(got['best_lp'][par], st['best_lp'])
    assert np.array_equal(got['lam'][hpar], st['lam']) and np.array_equal(got['c0'][hpar], st['c0']) and got['step'][par] == STEP
    assert np.array_equal(got['cur'], st['cur']) and np.array_equal(got['seg'], st['seg'])
    keep = np.arange(NMCMC + 1) != STEP
    assert np.array_equal(got['lps'][:, keep], st['lps'][:, keep])
    keep = np.arange(NROUNDS + 1) != ROUND + 1
    assert np.array_equal(got['taus'][:, keep], st['taus'][:, keep])
    # equal inputs give equal bits; taus NULL changes nothing else; a chain alone is the chain among others
    again, bare = _gibbs(st, par, hpar), _gibbs(st, par, hpar, taus=False)
    for k in ('gcur', 'cur_lp', 'best_lp', 'lps', 'lam', 'c0', 'step'):
        assert np.array_equal(again[k], got[k]) and np.array_equal(bare[k], got[k]), k
    assert np.array_equal(again['taus'], got['taus'])
    for c in range(C):
        one = _gibbs(st, par, hpar, rows=[c])
        for k in ('gcur', 'lps', 'taus'):
            assert np.array_equal(one[k][0], got[k][c]), (k, c)
        for k in ('cur_lp', 'best_lp', 'lam', 'c0'):
            assert np.array_equal(one[k][:, 0], got[k][:, c]), (k, c)


@pytest.mark.parametrize("name", list(SHAPES))
def test_gibbs_round_leaves_a_chain_with_a_nan_alone(name):
    st = _gibbs_state(name)
    clean = _gibbs(st, 1, 0)
    bad = dict(st, cur=st['cur'].copy())
    bad['cur'][1, st['seg'][2]] = np.nan
    got = _gibbs(bad, 1, 0)
    others = [c for c in range(st['C']) if c != 1]
    assert np.array_equal(got['lam'][1][1], st['lam'][1]) and got['c0'][1][1] == st['c0'][1]
    assert got['cur_lp'][0][1] == st['cur_lp'][1] and got['best_lp'][0][1] == st['best_lp'][1]
    assert np.array_equal(got['gcur'][1], st['gcur'][1]) and np.array_equal(got['lps'][1], st['lps'][1])
    assert np.array_equal(got['taus'][1, ROUND + 1], st['taus'][1, ROUND])        # the precisions in force are repeated
    for k in ('gcur', 'lps', 'taus'):
        assert np.array_equal(got[k][others], clean[k][others]), k
    for k in ('cur_lp', 'best_lp', 'lam', 'c0'):
        assert np.array_equal(got[k][:, others], clean[k][:, others]), k
    assert got['step'][0] == STEP


def test_every_refusal_returns_einval_with_a_message():
    L = _lib.lib()
    st = _gibbs_state("p37")
    t = {k: _dev(v) for k, v in dict(cur=st['cur'], gcur=st['gcur'], cur_lp=np.stack([st['cur_lp']] * 2),
                                     best_lp=np.stack([st['best_lp']] * 2), lps=st['lps'], lam=np.stack([st['lam']] * 2),
                                     c0=np.stack([st['c0']] * 2), seg=st['seg'], taus=st['taus'],
                                     step=np.array([STEP, STEP])).items()}
    before = {k: v.clone() for k, v in t.items()}
    ptrs = ['cur', 'gcur', 'cur_lp', 'best_lp', 'lps', 'lam', 'c0', 'seg', 'taus', 'step']
    base = dict(sigma=SIGMA, a0=A0, b0=B0, G=st['G'], round=ROUND, nrounds=NROUNDS, C=st['C'], chain0=CHAIN0, p=st['p'],
                nmcmc=NMCMC, seed=SEED, parity=0, hyper_parity=0)
    cases = [dict(a0=0.0), dict(a0=-1.0), dict(a0=np.inf), dict(a0=np.nan), dict(b0=0.0), dict(b0=np.inf), dict(b0=np.nan),
             dict(sigma=0.0), dict(sigma=-0.3), dict(sigma=np.inf), dict(sigma=np.nan), dict(G=0), dict(G=33), dict(C=0),
             dict(C=65536), dict(p=0), dict(round=-1), dict(round=NROUNDS), dict(parity=2), dict(parity=-1),
             dict(hyper_parity=2)] + [dict(null=k) for k in ptrs if k != 'taus']
    for case in cases:
        kw = dict(base, **{k: v for k, v in case.items() if k != 'null'})
        a = [None if case.get('null') == k else t[k].data_ptr() for k in ptrs]
        rc = L.qn_hyper_gibbs(*a, kw['sigma'], kw['a0'], kw['b0'], kw['G'], kw['round'], kw['nrounds'], kw['C'], kw['chain0'],
                              kw['p'], kw['nmcmc'], kw['seed'], kw['parity'], kw['hyper_parity'], None)
        msg = L.qn_last_error().decode()
        assert rc == _lib.CONSTANTS['QN_EINVAL'] and msg.startswith("qn_hyper_gibbs:"), (case, rc, msg)
    W, lam, c0, seg, g = t['cur'], t['lam'][0], t['c0'][0], t['seg'], t['gcur']
    sse = torch.zeros(st['C'], dtype=torch.float64, device="cuda")
    ok = dict(W=W.data_ptr(), lam=lam.data_ptr(), c0=c0.data_ptr(), seg=seg.data_ptr(), G=st['G'], grad=g.data_ptr(),
              gdtype=_lib.QN_F64, sse=sse.data_ptr(), stride=1, C=st['C'], p=st['p'])
    for case in [dict(W=None), dict(lam=None), dict(c0=None), dict(seg=None), dict(grad=None, sse=None), dict(G=0), dict(G=33),
                 dict(C=0), dict(C=65536), dict(p=0), dict(stride=0), dict(gdtype=7)]:
        kw = dict(ok, **case)
        rc = L.qn_prior_fold_g(kw['W'], kw['lam'], kw['c0'], kw['seg'], kw['G'], kw['grad'], kw['gdtype'], kw['sse'], kw['stride'],
                               kw['C'], kw['p'], None)
        msg = L.qn_last_error().decode()
        assert rc == _lib.CONSTANTS['QN_EINVAL'] and msg.startswith("qn_prior_fold_g:"), (case, rc, msg)
    torch.cuda.synchronize()
    for k in t:                                                                # before any pointer is touched
        assert torch.equal(t[k], before[k]), k
    assert torch.equal(sse, torch.zeros_like(sse))


# ------------------------------------------------------------------------------------------------ the sampler
def _solver(hidden):
    from quinn_amd.nns.mlp import MLP
    from quinn_amd.solvers.nn_mcmc import NN_MCMC
    torch.manual_seed(0)
    return NN_MCMC(MLP(1, 1, hidden, activ="tanh"), verbose=False, kernels="float64")


def _within_5_se(per_chain, exact, what):
    """per_chain [C, k]: the chains' time averages of k statistics.  The chains are independent, so the mean over chains lies
    within 5 (std over chains / sqrt(C)) of the exact value, whatever the autocorrelation within a chain."""
    C = per_chain.shape[0]
    mean, se = per_chain.mean(axis=0), per_chain.std(axis=0, ddof=1) / np.sqrt(C)
    print(what, "exact", exact, "z", (mean - exact) / se)
    assert np.all(np.abs(mean - exact) <= 5 * se), (what, mean, se)


def _flat_run(hyperprior, ini_scale):
    """MLP(1, 1, (4,)) (p = 13) on N = 8 rows with datanoise = 1e6: the likelihood is flat to rounding, the posterior is the
    prior.  256 chains, 600 HMC steps (L = 5, epsilon = 0.3), the first 100 burned; starts ~ N(0, ini_scale^2 I)."""
    uq = _solver((4,))
    assert uq.pdim == 13
    rs = np.random.RandomState(0)
    x = rs.rand(8, 1) * 2 - 1
    y = np.sin(3 * x) + 0.1 * rs.randn(8, 1)
    C = 256
    uq.fit(x, y, zflag=False, datanoise=1e6, nmcmc=600, param_ini=ini_scale * rs.randn(C, 13), sampler='hmc',
           sampler_params={'epsilon': 0.3, 'L': 5}, seeds=range(C), engine='device', hyperprior=hyperprior)
    r = uq.mcmc_results
    assert np.isfinite(r['chain']).all() and np.isfinite(r['logpost']).all()
    print("accrate", np.mean(r['accrate']))
    assert np.mean(r['accrate']) > 0.5
    return r


def test_the_sampler_samples_the_model():
    """Exact under the prior: E[tau_g] = a0 / b0 = 1, E[w_j^2] = E[1 / tau] = b0 / (a0 - 1) = 1.5, E[w_j] = 0."""
    r = _flat_run(dict(a0=3, b0=3, groups='layer'), 1.0)
    assert r['tau'].shape == (256, 601, 2) and r['prior_groups'] == [('layer0', 0, 8), ('layer1', 8, 13)]
    w = r['chain'][:, 100:]
    _within_5_se(r['tau'][:, 100:].mean(axis=1), 1.0, "E[tau_g]")
    _within_5_se((w ** 2).mean(axis=1), 1.5, "E[w_j^2]")
    _within_5_se(w.mean(axis=1), 0.0, "E[w_j]")


def test_every_0_samples_the_fixed_per_group_scales():
    """Fixed tau = 4: w ~ N(0, 1 / 4).  The chains start in that law: at fixed tau a trajectory of L epsilon sqrt(tau) = 3.0 rad
    is almost a half period, q -> -q, so w_j^2 forgets a start of another scale only over ~50 steps (from N(0, I) the run passes
    too, with every z between 1.2 and 4.7, all of one sign)."""
    r = _flat_run(dict(a0=3, b0=3, groups='layer', every=0, tau0=4), 0.5)
    assert r['tau'].shape == (256, 1, 2) and np.all(r['tau'] == 4.0)
    w = r['chain'][:, 100:]
    _within_5_se((w ** 2).mean(axis=1), 0.25, "E[w_j^2]")
    _within_5_se(w.mean(axis=1), 0.0, "E[w_j]")


def _problem(seed=0, N=48):
    rs = np.random.RandomState(seed)
    x = rs.rand(N, 1) * 6 - 3
    return x, np.sin(x).sum(axis=1, keepdims=True) + 0.1 * rs.randn(N, 1)


HP = dict(a0=2.0, b0=1.0, groups='tensor', every=2)


def _fit(sampler_params, C=8, nmcmc=60, **kw):
    x, y = _problem(seed=2, N=64)
    uq = _solver((6,))
    inis = np.stack([0.1 * np.random.RandomState(30 + c).randn(uq.pdim) for c in range(C)])
    uq.fit(x, y, zflag=False, datanoise=0.3, nmcmc=nmcmc, param_ini=inis, sampler='hmc', sampler_params=sampler_params,
           seeds=range(C), engine='device', hyperprior=HP, **kw)
    return uq, inis


@pytest.fixture(scope="module")
def fitted():
    return _fit({'epsilon': 0.01, 'L': 3}, diagnostics=True)


def test_through_the_solver(fitted):
    uq, inis = fitted
    r = uq.mcmc_results
    C, T, G = 8, 61, 4
    assert r['tau'].shape == (C, 60 // 2 + 1, G) and np.all(r['tau'] > 0) and np.all(r['tau'][:, 0] == 2.0)     # a0 / b0
    assert r['prior_groups'] == [('W0', 0, 6), ('b0', 6, 12), ('W1', 12, 18), ('b1', 18, 19)]
    assert uq.lpinfo['lparams']['hyperprior'] == dict(HP, tau0=None)
    assert uq.samples.shape == (C, T, uq.pdim) and np.isfinite(uq.samples).all()
    assert 0.0 < np.mean(r['accrate']) <= 1.0 and not np.array_equal(r['tau'][:, 1], r['tau'][:, 0])
    assert np.shape(uq.diagnostics['logpost']['rhat']) == (1,)
    # logpost[c, t] is the joint density of the stored row and the precisions in force: those of round t // every
    seg = np.array([0, 6, 12, 18, 19])
    bare = dict(uq.lpinfo, lparams={'sigma': 0.3})
    loglik = uq.logpost_batch(uq.samples.reshape(-1, uq.pdim), bare).reshape(C, T)
    tau_t = r['tau'][:, np.arange(T) // 2]                                    # [C, T, G]
    want = np.stack([hy.log_joint(uq.samples[:, t], tau_t[:, t], seg, HP['a0'], HP['b0'], loglik=loglik[:, t]) for t in range(T)], axis=1)
    np.testing.assert_allclose(r['logpost'], want, rtol=1e-9)
    assert uq.predict_ens(np.linspace(-1, 1, 5)[:, None], nens=4, nburn=20, chain='all').shape == (4, 5, 1)


def test_a_run_is_reproducible_and_a_chain_does_not_depend_on_the_split(fitted):
    uq, inis = fitted
    r = uq.mcmc_results
    again = _fit({'epsilon': 0.01, 'L': 3})[0].mcmc_results
    for k in ('chain', 'logpost', 'alphas', 'accrate', 'mapparams', 'maxpost', 'tau'):
        assert np.array_equal(again[k], r[k]), k
    op = uq._operator(uq.lpinfo)
    old = op.set_plan_batch(8)                  # split every chain's rows as the launch of all eight chains does
    try:
        half = DeviceHMC(op, 0.3, epsilon=0.01, L=3, seed=0, chain0=4, hyperprior=HP).run(60, inis[4:])
    finally:
        op.set_plan_batch(old)
    for k, key in (('chain', 'chain'), ('logpost', 'logpost'), ('tau', 'tau'), ('maxpost', 'maxpost')):
        assert np.array_equal(half[key].cpu().numpy(), r[k][4:]), k
    two = _fit({'epsilon': 0.01, 'L': 3, 'groups': 2})[0].mcmc_results
    for k in ('chain', 'logpost', 'tau'):
        assert np.array_equal(two[k], r[k]), k


def test_warm_up_runs_with_the_gibbs_rounds_and_returns_the_step_sizes():
    uq, _ = _fit({'epsilon': 0.01, 'L': 3, 'adapt': 20})
    r = uq.mcmc_results
    assert r['epsilon'].shape == (8,) and np.all(r['epsilon'] > 0) and r['nwarm'] == 20
    assert r['tau'].shape == (8, 31, 4) and np.isfinite(r['logpost']).all() and np.all(r['tau'] > 0)
    from quinn_amd.mcmc.device_mala import DeviceMALA
    op = uq._operator(uq.lpinfo)
    m = DeviceMALA(op, 0.3, epsilon=0.01, seed=0, hyperprior=HP).run(20, np.zeros((4, uq.pdim)) + 0.1)
    assert m['tau'].shape == (4, 11, 4) and torch.isfinite(m['logpost']).all()
