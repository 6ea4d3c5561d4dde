"""GPU: the sampled noise level of the device HMC / MALA engines.  qn_noise_fold against `noise.fold_n` (gradient bit for bit,
SSE to 1e-13), against qn_prior_fold_g at kappa = 1, d0 = 0, alone and among other chains, with non-finite rows; qn_noise_gibbs
against `noise.gibbs_round` at both values of both parities with every slot it must not touch checked, and the refusals of
both; a frozen noise level against a plain run at that level; the sampler against the exact conditional moments; and the path
through `NN_MCMC.fit`, `noise_samples` and `score`."""
import numpy as np
import pytest
import torch

from quinn_amd import _lib, scoring
from quinn_amd.mcmc import hyper as hy
from quinn_amd.mcmc import noise as nz
from quinn_amd.mcmc.device_hmc import DeviceHMC

pytestmark = pytest.mark.gpu

# (C, p, seg) of test_gpu_hyper.py -- a one-element group and odd boundaries; boundaries that straddle a workgroup's chunk of a
# 2500-element row -- and the same rows without a weight prior (G = 0)
SHAPES = {"p37": (3, 37, [0, 5, 6, 30, 37]), "p2500": (2, 2500, [0, 1023, 1025, 2500]), "p37_g0": (3, 37, None),
          "p2500_g0": (2, 2500, None)}
GROUPED = ["p37", "p2500"]
SIGMA, A0, B0, N_ROWS, N_OUT = 0.3, 2.0, 1.5, 16, 2
N_ENT = N_ROWS * N_OUT
EPS = 2.0 ** -52


def _dev(a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def _ptr(t):
    return None if t is None else t.data_ptr()


def _seg(seg):
    return None if seg is None else np.asarray(seg, dtype=np.int64)


def _fold(W, kappa, d0, lam, c0, seg, grad=None, sse=None, stride=1):
    """qn_noise_fold through the C ABI on copies of grad / sse -> (grad', sse') numpy, None for None."""
    Wt, kt, dt, lt, ct, st_ = _dev(W), _dev(kappa), _dev(d0), _dev(lam), _dev(c0), _dev(_seg(seg))
    gt, st = _dev(grad), _dev(sse)
    gdt = _lib.QN_F32 if gt is not None and gt.dtype == torch.float32 else _lib.QN_F64
    C, p = Wt.shape
    G = 0 if seg is None else len(seg) - 1
    _lib.check(_lib.lib().qn_noise_fold(Wt.data_ptr(), kt.data_ptr(), dt.data_ptr(), _ptr(lt), _ptr(ct), _ptr(st_), G, _ptr(gt),
                                        gdt, _ptr(st), stride, C, p, None), "qn_noise_fold")
    torch.cuda.synchronize()
    assert np.array_equal(Wt.cpu().numpy(), W, equal_nan=True) and np.array_equal(kt.cpu().numpy(), kappa)
    return (None if gt is None else gt.cpu().numpy()), (None if st is None else st.cpu().numpy())


def _fold_inputs(name):
    C, p, seg = SHAPES[name]
    rs = np.random.RandomState(p)
    W, g, sse1, sse3 = rs.randn(C, p), 3.0 * rs.randn(C, p), 10.0 + 40.0 * rs.rand(C), 10.0 + 40.0 * rs.rand(C, 3)
    lam, c0 = (0.2 + rs.rand(C, len(seg) - 1), rs.randn(C)) if seg is not None else (None, None)
    return C, p, seg, W, g, sse1, sse3, lam, c0, 0.3 + rs.rand(C), 5.0 * rs.randn(C)


@pytest.mark.parametrize("name", list(SHAPES))
def test_noise_fold_equals_the_numpy_fold(name):
    C, p, seg, W, g64, sse1, sse3, lam, c0, kappa, d0 = _fold_inputs(name)
    for g in (g64, g64.astype(np.float32)):
        want_g, want_s = nz.fold_n(W, kappa, d0, lam, c0, seg, grad=g, sse=sse1)
        got_g, none = _fold(W, kappa, d0, lam, c0, seg, grad=g)               # sse NULL
        assert none is None and got_g.dtype == g.dtype
        assert np.array_equal(got_g, want_g)                                 # the same roundings: bit for bit
        got_g2, got_s = _fold(W, kappa, d0, lam, c0, seg, grad=g, sse=sse1)
        assert np.array_equal(got_g2, want_g)
        print(name, g.dtype, "sse rel err", np.abs(got_s - want_s) / np.abs(want_s))
        assert np.all(np.abs(got_s - want_s) <= 1e-13 * np.abs(want_s))
        assert np.array_equal(_fold(W, kappa, d0, lam, c0, seg, sse=sse1)[1], got_s)     # grad NULL: the same sum, another grid
        again = _fold(W, kappa, d0, lam, c0, seg, grad=g, sse=sse1)
        assert np.array_equal(again[0], got_g2) and np.array_equal(again[1], got_s)
    # sse_stride = 3: column 0 receives the fold, the other columns are unchanged bit for bit
    got3 = _fold(W, kappa, d0, lam, c0, seg, sse=sse3, stride=3)[1]
    assert np.array_equal(got3[:, 1:], sse3[:, 1:])
    want3 = nz.fold_n(W, kappa, d0, lam, c0, seg, sse=sse3[:, 0])[1]
    assert np.all(np.abs(got3[:, 0] - want3) <= 1e-13 * np.abs(want3))
    assert np.array_equal(got3[:, 0], _fold(W, kappa, d0, lam, c0, seg, sse=np.ascontiguousarray(sse3[:, 0]))[1])


@pytest.mark.parametrize("name", GROUPED)
def test_noise_fold_at_kappa_1_d0_0_is_the_per_group_fold_bit_for_bit(name):
    C, p, seg, W, g64, sse1, _, lam, c0, _, _ = _fold_inputs(name)
    L = _lib.lib()
    for g in (g64, g64.astype(np.float32)):
        got_g, got_s = _fold(W, np.ones(C), np.zeros(C), lam, c0, seg, grad=g, sse=sse1)
        Wt, lt, ct, st_, gt, st = _dev(W), _dev(lam), _dev(c0), _dev(_seg(seg)), _dev(g), _dev(sse1)
        gdt = _lib.QN_F32 if gt.dtype == torch.float32 else _lib.QN_F64
        _lib.check(L.qn_prior_fold_g(Wt.data_ptr(), lt.data_ptr(), ct.data_ptr(), st_.data_ptr(), len(seg) - 1, gt.data_ptr(), gdt,
                                     st.data_ptr(), 1, C, p, None), "qn_prior_fold_g")
        torch.cuda.synchronize()
        assert np.array_equal(got_g, gt.cpu().numpy()) and np.array_equal(got_s, st.cpu().numpy())


@pytest.mark.parametrize("name", list(SHAPES))
def test_noise_fold_a_chain_alone_is_the_chain_among_others_and_non_finite_rows_stay_home(name):
    C, p, seg, W, g64, sse1, _, lam, c0, kappa, d0 = _fold_inputs(name)

    def rows(a, c):
        return None if a is None else a[c:c + 1]
    for g in (g64, g64.astype(np.float32)):
        whole = _fold(W, kappa, d0, lam, c0, seg, grad=g, sse=sse1)
        for c in range(C):
            one = _fold(W[c:c + 1], kappa[c:c + 1], d0[c:c + 1], rows(lam, c), rows(c0, c), seg, grad=g[c:c + 1], sse=sse1[c:c + 1])
            assert np.array_equal(one[0][0], whole[0][c]) and one[1][0] == whole[1][c]
    clean_g, clean_s = _fold(W, kappa, d0, lam, c0, seg, grad=g64, sse=sse1)
    others = [c for c in range(C) if c != 1]
    j = 5 if seg is None else seg[1]
    for bad, check in ((np.inf, lambda v: v == np.inf), (np.nan, np.isnan)):
        Wb = W.copy()
        Wb[1, j] = bad
        got_g, got_s = _fold(Wb, kappa, d0, lam, c0, seg, grad=g64, sse=sse1)
        if seg is not None:                                                   # (without a prior the weights do not enter)
            assert check(got_s[1]), (bad, got_s)
        assert np.array_equal(got_s[others], clean_s[others]) and np.array_equal(got_g[others], clean_g[others])
        mask = np.arange(p) != j
        assert np.array_equal(got_g[1, mask], clean_g[1, mask])
    sb = sse1.copy()
    sb[1] = np.nan                                                            # a non-finite SSE stays in its chain too
    got_s = _fold(W, kappa, d0, lam, c0, seg, sse=sb)[1]
    assert np.isnan(got_s[1]) and np.array_equal(got_s[others], clean_s[others])


# ------------------------------------------------------------------------------------------------ the Gibbs round
CHAIN0, SEED, STEP, NMCMC, NROUNDS, ROUND = 5, 77, 6, 9, 4, 2


def _gibbs_state(name, seed=0):
    """A state built from a KNOWN data SSE: folded as the engine folds it, cur_lp = -(h sse' + lik_const)."""
    C, p, seg = SHAPES[name]
    rs = np.random.RandomState(1000 + p + seed)
    seg = _seg(seg)
    cur, sse = rs.randn(C, p), 10.0 + 40.0 * rs.rand(C)
    lam = c0 = None
    if seg is not None:
        lam, c0 = hy.fold_constants_g(SIGMA, 0.5 + rs.rand(C, len(seg) - 1), seg, 3.0, 2.0)
    s2 = SIGMA ** 2 * np.exp(0.5 * rs.randn(C))
    kappa, d0 = nz.fold_constants_n(SIGMA, s2, N_ENT, N_ROWS, A0, B0)
    gcur, fsse = nz.fold_n(cur, kappa, d0, lam, c0, seg, grad=3.0 * rs.randn(C, p), sse=sse)
    h, lik_const = nz.lik_constants(SIGMA, N_ROWS)
    sig = rs.rand(C, NROUNDS + 1)
    sig[:, ROUND] = np.sqrt(s2)
    return dict(C=C, p=p, G=0 if seg is None else len(seg) - 1, seg=seg, cur=cur, gcur=gcur, lam=lam, c0=c0, kappa=kappa, d0=d0,
                sse=sse, cur_lp=-(h * fsse + lik_const), best_lp=rs.randn(C), lps=rs.randn(C, NMCMC + 1), sig=sig)


def _want(st):
    return nz.gibbs_round(st['cur'], st['gcur'], st['cur_lp'], st['kappa'], st['d0'], SIGMA, N_ENT, N_ROWS, A0, B0, SEED, STEP,
                          CHAIN0, st['lam'], st['c0'], st['seg'])


def _gibbs(st, par, npar, rows=None, sig=True):
    """qn_noise_gibbs on device copies of the state (chains `rows`), slot par / npar current, the other slots filled with
    sentinels -> dict of numpy arrays after the launch."""
    rows = np.arange(st['C']) if rows is None else np.asarray(rows)
    C, G, p = len(rows), st['G'], st['p']

    def two(cur, sentinel, slot):
        a = np.full((2,) + cur.shape, sentinel, dtype=np.float64)
        a[slot] = cur
        return a
    t = {'cur': _dev(st['cur'][rows]), 'gcur': _dev(st['gcur'][rows]), 'cur_lp': _dev(two(st['cur_lp'][rows], -1.5, par)),
         'best_lp': _dev(two(st['best_lp'][rows], -2.5, par)), 'lps': _dev(st['lps'][rows]),
         'kappa': _dev(two(st['kappa'][rows], -3.5, npar)), 'd0': _dev(two(st['d0'][rows], -4.5, npar)),
         'lam': None if G == 0 else _dev(st['lam'][rows]), 'c0': None if G == 0 else _dev(st['c0'][rows]), 'seg': _dev(st['seg']),
         'sig': _dev(st['sig'][rows]) if sig else None, 'sse_rec': _dev(np.full(C, -5.5)) if sig else None}
    step = np.full(2, -9, dtype=np.int64)
    step[par] = STEP
    t['step'] = _dev(step)
    rc = _lib.lib().qn_noise_gibbs(t['cur'].data_ptr(), t['gcur'].data_ptr(), t['cur_lp'].data_ptr(), t['best_lp'].data_ptr(),
                                   t['lps'].data_ptr(), t['kappa'].data_ptr(), t['d0'].data_ptr(), _ptr(t['lam']), _ptr(t['c0']),
                                   _ptr(t['seg']), _ptr(t['sig']), _ptr(t['sse_rec']), t['step'].data_ptr(), SIGMA, A0, B0, N_ROWS, N_ENT, G,
                                   ROUND, NROUNDS, C, CHAIN0 + int(rows[0]), p, NMCMC, SEED, par, npar, None)
    _lib.check(rc, "qn_noise_gibbs")
    torch.cuda.synchronize()
    return {k: (None if v is None else v.cpu().numpy()) for k, v in t.items()}


def _close(got, want, rtol, what):
    """Elementwise: every entry within rtol of its own reference value."""
    err = np.abs(got - want) / np.abs(want)
    print(what, "max elementwise rel err", err.max())
    assert np.all(np.abs(got - want) <= rtol * np.abs(want)), (what, err.max())


def _ulps(got, want):
    return np.abs(got - want) / np.spacing(np.abs(want))


@pytest.mark.parametrize("name", list(SHAPES))
@pytest.mark.parametrize("par,npar", [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_noise_gibbs_equals_the_numpy_round(name, par, npar):
    """The state is built from a known data SSE; the SSE the KERNEL recovered (its optional sse_rec output) must lie within the
    cancellation bound of the inversion, 16 eps ((|cur_lp| + |lik_const|) / h + |d0| + |P|) / kappa, which on these states is
    below 1e-9 of the SSE (checked here); `noise.recover_sse`, the numpy restatement, is held to the same bound.  Every other
    output is compared with `noise.gibbs_round` entry by entry: 1e-12 relative, grad_cur 4 ulp."""
    st = _gibbs_state(name)
    C, G = st['C'], st['G']
    want = _want(st)
    assert want['ok'].all()
    h, lik_const = nz.lik_constants(SIGMA, N_ROWS)
    P = nz._prior_term(st['cur'], st['lam'], st['c0'], st['seg'])
    bound = 16 * EPS * ((np.abs(st['cur_lp']) + abs(lik_const)) / h + np.abs(st['d0']) + np.abs(P)) / st['kappa']
    print(name, "recovered SSE err", np.abs(want['sse'] - st['sse']), "bound", bound)
    assert np.all(bound < 1e-9 * st['sse']) and np.all(np.abs(want['sse'] - st['sse']) <= bound)
    got = _gibbs(st, par, npar)
    print(name, "kernel's recovered SSE err", np.abs(got['sse_rec'] - st['sse']))
    assert np.all(np.abs(got['sse_rec'] - st['sse']) <= bound)
    # the new slots (`gamma_draw` is the authority; the device log / sqrt / cos differ in the last bits)
    _close(got['sig'][:, ROUND + 1], want['sigma'], 1e-12, "sig")
    _close(got['kappa'][1 - npar], want['kappa'], 1e-12, "kappa'")
    _close(got['d0'][1 - npar], want['d0'], 1e-12, "d0'")
    _close(got['cur_lp'][1 - par], want['cur_lp'], 1e-12, "cur_lp'")
    _close(got['lps'][:, STEP], want['cur_lp'], 1e-12, "lps[:, t]")
    assert np.array_equal(got['lps'][:, STEP], got['cur_lp'][1 - par])
    print(name, "grad_cur max ulp", _ulps(got['gcur'], want['grad_cur']).max())
    assert np.all(_ulps(got['gcur'], want['grad_cur']) <= 4)                    # every entry, against the numpy round
    assert np.array_equal(got['best_lp'][1 - par], st['best_lp']) and got['step'][1 - par] == STEP
    # what the launch reads stays: slot par / npar of every double-buffered array, the state, every other stored entry
    assert np.array_equal(got['cur_lp'][par], st['cur_lp']) and np.array_equal(got['best_lp'][par], st['best_lp'])
    assert np.array_equal(got['kappa'][npar], st['kappa']) and np.array_equal(got['d0'][npar], st['d0']) and got['step'][par] == STEP
    assert np.array_equal(got['cur'], st['cur'])
    if G:
        assert np.array_equal(got['lam'], st['lam']) and np.array_equal(got['c0'], st['c0']) and np.array_equal(got['seg'], st['seg'])
    keep = np.arange(NMCMC + 1) != STEP
    assert np.array_equal(got['lps'][:, keep], st['lps'][:, keep])
    keep = np.arange(NROUNDS + 1) != ROUND + 1
    assert np.array_equal(got['sig'][:, keep], st['sig'][:, keep])
    # equal inputs give equal bits; sig NULL changes nothing else; a chain alone is the chain among others
    again, bare = _gibbs(st, par, npar), _gibbs(st, par, npar, sig=False)
    for k in ('gcur', 'cur_lp', 'best_lp', 'lps', 'kappa', 'd0', 'step'):
        assert np.array_equal(again[k], got[k]) and np.array_equal(bare[k], got[k]), k
    assert np.array_equal(again['sig'], got['sig']) and np.array_equal(again['sse_rec'], got['sse_rec'])
    for c in range(C):
        one = _gibbs(st, par, npar, rows=[c])
        for k in ('gcur', 'lps', 'sig', 'sse_rec'):
            assert np.array_equal(one[k][0], got[k][c]), (k, c)
        for k in ('cur_lp', 'best_lp', 'kappa', 'd0'):
            assert np.array_equal(one[k][:, 0], got[k][:, c]), (k, c)


@pytest.mark.parametrize("name", list(SHAPES))
def test_noise_gibbs_leaves_a_chain_with_a_nan_alone(name):
    """A NaN in cur (through the prior's sums) or, without a weight prior, in cur_lp; and a cached density so high that the
    recovered SSE is negative."""
    st = _gibbs_state(name)
    clean = _gibbs(st, 1, 0)
    others = [c for c in range(st['C']) if c != 1]
    for kind in ("nan", "negative"):
        bad = dict(st, cur=st['cur'].copy(), cur_lp=st['cur_lp'].copy())
        if kind == "nan" and st['G']:
            bad['cur'][1, st['seg'][2]] = np.nan
        elif kind == "nan":
            bad['cur_lp'][1] = np.nan
        else:
            bad['cur_lp'][1] = 1e7
        got = _gibbs(bad, 1, 0)
        assert got['kappa'][1][1] == st['kappa'][1] and got['d0'][1][1] == st['d0'][1]
        assert np.array_equal(got['cur_lp'][0][1], bad['cur_lp'][1], equal_nan=True) and got['best_lp'][0][1] == st['best_lp'][1]
        assert np.array_equal(got['gcur'][1], st['gcur'][1]) and np.array_equal(got['lps'][1], st['lps'][1])
        assert got['sig'][1, ROUND + 1] == st['sig'][1, ROUND]                    # the level in force is repeated
        for k in ('gcur', 'lps', 'sig'):
            assert np.array_equal(got[k][others], clean[k][others]), k
        for k in ('cur_lp', 'best_lp', 'kappa', 'd0'):
            assert np.array_equal(got[k][:, others], clean[k][:, others]), k
        assert got['step'][0] == STEP


def test_every_refusal_returns_einval_with_a_message():
    L = _lib.lib()
    st = _gibbs_state("p37")
    t = {k: _dev(v) for k, v in dict(cur=st['cur'], gcur=st['gcur'], cur_lp=np.stack([st['cur_lp']] * 2),
                                     best_lp=np.stack([st['best_lp']] * 2), lps=st['lps'], kappa=np.stack([st['kappa']] * 2),
                                     d0=np.stack([st['d0']] * 2), lam=st['lam'], c0=st['c0'], seg=st['seg'], sig=st['sig'],
                                     sse_rec=np.zeros(st['C']), step=np.array([STEP, STEP])).items()}
    before = {k: v.clone() for k, v in t.items()}
    ptrs = ['cur', 'gcur', 'cur_lp', 'best_lp', 'lps', 'kappa', 'd0', 'lam', 'c0', 'seg', 'sig', 'sse_rec', 'step']
    base = dict(sigma=SIGMA, a0=A0, b0=B0, n_rows=N_ROWS, n=N_ENT, G=st['G'], round=ROUND, nrounds=NROUNDS, C=st['C'], chain0=CHAIN0,
                p=st['p'], nmcmc=NMCMC, seed=SEED, parity=0, noise_parity=0)
    cases = [dict(a0=0.0), dict(a0=-1.0), dict(a0=np.inf), dict(a0=np.nan), dict(b0=0.0), dict(b0=np.inf), dict(b0=np.nan),
             dict(sigma=0.0), dict(sigma=-0.3), dict(sigma=np.inf), dict(sigma=np.nan), dict(G=-1), dict(G=33), dict(C=0),
             dict(C=65536), dict(p=0), dict(p=3), dict(chain0=-1), dict(nmcmc=0), dict(n_rows=0), dict(n=N_ROWS - 1),
             dict(round=-1), dict(round=NROUNDS), dict(nrounds=0), dict(parity=2), dict(parity=-1), dict(noise_parity=2)] + \
        [dict(null=k) for k in ptrs if k not in ('sig', 'sse_rec')]
    for case in cases:
        kw = dict(base, **{k: v for k, v in case.items() if k != 'null'})
        a = [None if case.get('null') == k else t[k].data_ptr() for k in ptrs]
        rc = L.qn_noise_gibbs(*a, kw['sigma'], kw['a0'], kw['b0'], kw['n_rows'], kw['n'], kw['G'], kw['round'], kw['nrounds'],
                              kw['C'], kw['chain0'], kw['p'], kw['nmcmc'], kw['seed'], kw['parity'], kw['noise_parity'], None)
        msg = L.qn_last_error().decode()
        assert rc == _lib.CONSTANTS['QN_EINVAL'] and msg.startswith("qn_noise_gibbs:"), (case, rc, msg)
    sse = torch.zeros(st['C'], dtype=torch.float64, device="cuda")
    ok = dict(W=t['cur'].data_ptr(), kappa=t['kappa'][0].data_ptr(), d0=t['d0'][0].data_ptr(), lam=t['lam'].data_ptr(),
              c0=t['c0'].data_ptr(), seg=t['seg'].data_ptr(), G=st['G'], grad=t['gcur'].data_ptr(), gdtype=_lib.QN_F64,
              sse=sse.data_ptr(), stride=1, C=st['C'], p=st['p'])
    for case in [dict(W=None), dict(kappa=None), dict(d0=None), dict(lam=None), dict(c0=None), dict(seg=None),
                 dict(grad=None, sse=None), dict(G=-1), dict(G=33), dict(C=0), dict(C=65536), dict(p=0), dict(p=3), dict(stride=0),
                 dict(gdtype=7)]:
        kw = dict(ok, **case)
        rc = L.qn_noise_fold(kw['W'], kw['kappa'], kw['d0'], kw['lam'], kw['c0'], kw['seg'], kw['G'], kw['grad'], kw['gdtype'],
                             kw['sse'], kw['stride'], kw['C'], kw['p'], None)
        msg = L.qn_last_error().decode()
        assert rc == _lib.CONSTANTS['QN_EINVAL'] and msg.startswith("qn_noise_fold:"), (case, rc, msg)
    torch.cuda.synchronize()
    for k in t:                                                                # before any pointer is touched
        assert torch.equal(t[k], before[k]), k
    assert torch.equal(sse, torch.zeros_like(sse))


# ------------------------------------------------------------------------------------------------ the sampler
def _solver(hidden, dtype="float64"):
    from quinn_amd.nns.mlp import MLP
    from quinn_amd.solvers.nn_mcmc import NN_MCMC
    torch.manual_seed(0)
    return NN_MCMC(MLP(1, 1, hidden, activ="tanh"), verbose=False, kernels="float64", dtype=dtype)


def _within_5_se(per_chain, exact, what):
    """per_chain [C]: the chains' time averages of a statistic.  The chains are independent, so the mean over chains lies
    within 5 (std over chains / sqrt(C)) of the exact value, whatever the autocorrelation within a chain."""
    C = per_chain.shape[0]
    mean, se = per_chain.mean(axis=0), per_chain.std(axis=0, ddof=1) / np.sqrt(C)
    print(what, "exact", exact, "mean", mean, "z", (mean - exact) / se)
    assert np.all(np.abs(mean - exact) <= 5 * se), (what, mean, se)


def _small_problem():
    rs = np.random.RandomState(0)
    x = rs.rand(8, 1) * 2 - 1
    return x, np.sin(3 * x) + 0.1 * rs.randn(8, 1), rs


def test_a_frozen_noise_level_is_a_plain_run_at_that_level():
    """every = 0, sigma_init = 2 datanoise: kappa = 1 / 4 is a power of two, so every scaled gradient and force equals the plain
    run's at 2 datanoise bit for bit, and so do the chains; the constant d0 enters the rounding of the accept ratio only (seed 0
    puts no accept decision within that rounding of its uniform).  Drives the fold through begin, leap and accept."""
    x, y, rs = _small_problem()
    s0, C = 0.1, 8
    ini = 0.3 * rs.randn(C, 13)
    runs = []
    for kw in (dict(datanoise=s0, noiseprior=dict(every=0, sigma_init=2 * s0)), dict(datanoise=2 * s0)):
        uq = _solver((4,))
        uq.fit(x, y, zflag=False, nmcmc=20, param_ini=ini, sampler='hmc', sampler_params={'epsilon': 0.02, 'L': 3},
               seeds=range(C), engine='device', **kw)
        runs.append(uq.mcmc_results)
    frozen, plain = runs
    assert frozen['sigma'].shape == (C, 1) and np.all(frozen['sigma'] == 2 * s0) and 'sigma' not in plain
    assert 0.0 < np.mean(plain['accrate']) and not np.array_equal(plain['chain'][:, -1], plain['chain'][:, 0])
    assert np.array_equal(frozen['chain'], plain['chain']) and np.array_equal(frozen['accrate'], plain['accrate'])
    np.testing.assert_allclose(frozen['logpost'], plain['logpost'], rtol=1e-12)
    np.testing.assert_allclose(frozen['maxpost'], plain['maxpost'], rtol=1e-12)


def test_the_gibbs_draw_samples_its_conditional():
    """priorsigma = 1e-6 pins the weights at 0, so SSE = sum y^2 to O(1e-6) and 1 / s2 ~ Gamma(a0 + n / 2, b0 + sum y^2 / 2):
    E[1 / s2] = shape / rate, E[s2] = rate / (shape - 1)."""
    x, y, rs = _small_problem()
    C, a0, b0 = 256, 3.0, 1.0
    uq = _solver((4,))
    uq.fit(x, y, zflag=False, datanoise=0.5, nmcmc=600, param_ini=np.zeros((C, 13)), sampler='hmc',
           sampler_params={'epsilon': 3e-7, 'L': 5}, seeds=range(C), engine='device', priorsigma=1e-6,
           noiseprior=dict(a0=a0, b0=b0))
    r = uq.mcmc_results
    assert r['sigma'].shape == (C, 601) and np.isfinite(r['sigma']).all() and np.isfinite(r['logpost']).all()
    assert np.abs(r['chain']).max() < 1e-4
    print("accrate", np.mean(r['accrate']))
    shape, rate = a0 + 0.5 * 8, b0 + 0.5 * float(np.sum(y * y))
    s2 = r['sigma'][:, 100:] ** 2
    _within_5_se((1.0 / s2).mean(axis=1), shape / rate, "E[1 / s2]")
    _within_5_se(s2.mean(axis=1), rate / (shape - 1.0), "E[s2]")


NP = dict(a0=3.0, b0=0.5)


def _fit(sampler_params, C=8, nmcmc=60, noiseprior=NP, **kw):
    rs = np.random.RandomState(2)
    x = rs.rand(32, 1) * 6 - 3
    y = np.sin(x) + 0.1 * rs.randn(32, 1)
    uq = _solver((6,))
    inis = np.stack([0.1 * np.random.RandomState(30 + c).randn(uq.pdim) for c in range(C)])
    uq.fit(x, y, zflag=False, datanoise=0.5, nmcmc=nmcmc, param_ini=inis, sampler='hmc', sampler_params=sampler_params,
           seeds=range(C), engine='device', noiseprior=noiseprior, **kw)
    return uq, inis, x, y


@pytest.fixture(scope="module")
def fitted():
    return _fit({'epsilon': 0.01, 'L': 3}, diagnostics=True)


def test_through_the_solver(fitted):
    """The round after step t conditions on stored row t (the state the step left) and writes sigma[:, t] (every = 1): the level
    row t + 1 is then drawn at.  So 1 / sigma[c, t]^2 | row t ~ Gamma(a0 + n / 2, rate b0 + SSE(row t) / 2), which is checked in
    the mean (Rao-Blackwell) and, draw by draw, against the contract's unit-rate variate of (seed, step t, chain c)."""
    uq, inis, x, y = fitted
    r = uq.mcmc_results
    C, T, n = 8, 61, 32
    assert r['sigma'].shape == (C, T) and np.isfinite(r['sigma']).all() and np.all(r['sigma'] > 0) and np.all(r['sigma'][:, 0] == 0.5)
    assert uq.lpinfo['lparams']['noiseprior'] == dict(NP, every=1, sigma_init=None)
    assert uq.samples.shape == (C, T, uq.pdim) and np.isfinite(uq.samples).all() and np.isfinite(r['logpost']).all()
    assert np.shape(uq.diagnostics['logpost']['rhat']) == (1,)
    op = uq._operator(uq.lpinfo)
    sse = op.sse(torch.as_tensor(uq.samples.reshape(-1, uq.pdim), device="cuda")).cpu().numpy().reshape(C, T)
    shape, rate = NP['a0'] + 0.5 * n, NP['b0'] + 0.5 * sse
    prec = 1.0 / r['sigma'] ** 2
    diff = prec[:, 20:].mean(axis=1) - (shape / rate[:, 20:]).mean(axis=1)
    _within_5_se(diff, 0.0, "Rao-Blackwell: mean 1 / sigma_t^2 - mean shape / rate(row t)")
    unit = np.stack([hy.gamma_draw(0, t, np.arange(C), 0, shape, 1.0, purpose=nz.PURPOSE_NOISE) for t in range(1, T)], axis=1)
    np.testing.assert_allclose(prec[:, 1:] * rate[:, 1:], unit, rtol=1e-8)
    # logpost[c, t] is the joint density of row t and the level in force after its round: sigma[:, t]
    np.testing.assert_allclose(r['logpost'], nz.log_joint(sse, r['sigma'] ** 2, n, NP['a0'], NP['b0']), rtol=1e-9)
    # noise_samples is aligned with the rows predict_ens picks
    rows = [20 + j * 10 for j in range(4)]
    assert np.array_equal(uq.noise_samples(nens=4, nburn=20, chain=3), r['sigma'][3, rows])
    pooled = uq.noise_samples(nens=16, nburn=20, chain='all')
    assert np.array_equal(pooled, np.concatenate([r['sigma'][c, [20, 40]] for c in range(C)]))
    # score at the sampled levels: another predictive than at the nominal 0.5, and pred_score with V built by hand
    xt = np.linspace(-3, 3, 9)[:, None]
    yt = np.sin(xt)
    own = uq.score(xt, yt, nsam=16, nburn=20, chain='all')
    nominal = uq.score(xt, yt, noise=0.5, nsam=16, nburn=20, chain='all')
    assert own['nlpd'] != nominal['nlpd'] and not np.allclose(own['lppd_k'], nominal['lppd_k'])
    F = uq.predict_ens(xt, nens=16, nburn=20, chain='all')
    hand = scoring.pred_score(F, yt, 0.0, V=np.broadcast_to((pooled ** 2)[:, None, None], F.shape))
    for k in ('lppd_k', 'p_waic_k', 'pit', 'crps_k', 'mean', 'var'):
        np.testing.assert_allclose(own[k], hand[k], rtol=1e-12, atol=1e-14, err_msg=k)
    assert own['nlpd'] == pytest.approx(hand['nlpd'], rel=1e-12)


def test_a_run_is_reproducible_and_a_chain_does_not_depend_on_the_split(fitted):
    uq, inis, _, _ = fitted
    r = uq.mcmc_results
    again = _fit({'epsilon': 0.01, 'L': 3})[0].mcmc_results
    for k in ('chain', 'logpost', 'alphas', 'accrate', 'mapparams', 'maxpost', 'sigma'):
        assert np.array_equal(again[k], r[k]), k
    op = uq._operator(uq.lpinfo)
    old = op.set_plan_batch(8)                  # split every chain's rows as the launch of all eight chains does
    try:
        half = DeviceHMC(op, 0.5, epsilon=0.01, L=3, seed=0, chain0=4, noiseprior=NP).run(60, inis[4:])
    finally:
        op.set_plan_batch(old)
    for k, key in (('chain', 'chain'), ('logpost', 'logpost'), ('sigma', 'sigma'), ('maxpost', 'maxpost')):
        assert np.array_equal(half[key].cpu().numpy(), r[k][4:]), k
    two = _fit({'epsilon': 0.01, 'L': 3, 'groups': 2})[0].mcmc_results
    for k in ('chain', 'logpost', 'sigma'):
        assert np.array_equal(two[k], r[k]), k


def test_warm_up_and_a_hyper_prior_run_with_the_noise_rounds():
    uq, _, _, _ = _fit({'epsilon': 0.01, 'L': 3, 'adapt': 20}, hyperprior=dict(a0=3, b0=3, groups='layer'))
    r = uq.mcmc_results
    assert r['epsilon'].shape == (8,) and np.all(r['epsilon'] > 0) and np.isfinite(r['epsilon']).all() and r['nwarm'] == 20
    assert r['tau'].shape == (8, 61, 2) and np.isfinite(r['tau']).all() and np.all(r['tau'] > 0)
    assert r['sigma'].shape == (8, 61) and np.isfinite(r['sigma']).all() and np.all(r['sigma'] > 0)
    assert np.isfinite(r['logpost']).all() and np.isfinite(r['chain']).all()
    from quinn_amd.mcmc.device_mala import DeviceMALA
    op = uq._operator(uq.lpinfo)
    m = DeviceMALA(op, 0.5, epsilon=0.01, seed=0, priorsigma=2.0, noiseprior=dict(NP, every=2)).run(20, np.zeros((4, uq.pdim)) + 0.1)
    assert m['sigma'].shape == (4, 11) and torch.isfinite(m['logpost']).all() and torch.isfinite(m['sigma']).all()


def test_refusals_through_the_solver_and_the_engine():
    x, y, _ = _small_problem()
    base = dict(zflag=False, datanoise=0.1, nmcmc=4, param_ini=np.zeros((2, 13)), seeds=[0, 1], noiseprior=dict(a0=3, b0=1))
    for kw in (dict(sampler='amcmc', engine='device', sampler_params={}), dict(sampler='hmc', engine='host', sampler_params={}),
               dict(sampler='nuts', engine='device', sampler_params={}),
               dict(sampler='hmc', engine='device', sampler_params={'ladder': 2}),
               dict(sampler='hmc', engine='device', sampler_params={'use_graph': True}),
               dict(sampler='hmc', engine='device', sampler_params={}, noiseprior=dict(a0=3))):
        with pytest.raises(ValueError, match="noiseprior"):
            _solver((4,)).fit(x, y, **dict(base, **kw))
    with pytest.raises(ValueError, match="noiseprior"):
        _solver((4,), dtype="float32").fit(x, y, sampler='hmc', engine='device', sampler_params={}, **base)
    import inspect
    from quinn_amd.solvers.nn_mcmc import NN_MCMC
    assert inspect.signature(NN_MCMC.fit).parameters['noiseprior'].kind is inspect.Parameter.KEYWORD_ONLY
