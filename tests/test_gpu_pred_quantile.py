"""GPU: `qn_pred_quantile` (csrc/qn_quantile.hip) against its numpy contract (`quinn_amd/predquant.py`), against the independent
PIT kernels it inverts (`qn_pred_score`, `qn_pred_score_w`), its isolation and reproducibility properties, and the solver surface.

Bounds.  Empirical mode with equal weights: the contract's bits (sorting and one two-sided interpolation round alike).  With
weights: rtol = 1e-9 scaled by max |F|, the tolerance of tests/test_gpu_rank_diag.py -- the running weight sum is taken in another
fixed order (per-thread chunks), which moves a position by about M eps ~ 2e-13 and the quantile by that times the gap between two
neighbours over the width of their positions.  Mixture mode: the residual bound of the contract, |G(y) - q| <= (M + 16) eps +
2 spacing(|y|) g(y), evaluated by the contract at the kernel's y; and on unimodal entries rtol = 1e-9 against the contract's y
(the two differ by the rounding of G, M eps, over the density: about 1e-13 relative here).  Every comparison prints the largest
deviation it saw before it asserts."""
import numpy as np
import pytest
import torch

from quinn_amd import _lib, scoring
from quinn_amd import predquant as pq
from test_pred_quantile_cpu import EMP_LEVELS, MIX_LEVELS, MS, bits, mixture_residual, quant_inputs, quant_weights

pytestmark = pytest.mark.gpu

KQ = [(1, 1), (5, 3), (67, 8)]
RTOL = 1e-9


def device_rows(F, q, sigma, V=None, wm=None, return_iters=False):
    Ft = torch.as_tensor(np.ascontiguousarray(F)).cuda()
    Vt = None if V is None else torch.as_tensor(np.ascontiguousarray(V)).cuda()
    wt = None if wm is None else torch.as_tensor(np.ascontiguousarray(wm, dtype=np.float64)).cuda()
    out = scoring.quantile_rows(Ft, q, sigma, Vt, wt, return_iters=return_iters)
    if return_iters:
        return out[0].cpu().numpy(), out[1].cpu().numpy()
    return out.cpu().numpy()


@pytest.mark.parametrize("kq", KQ, ids=lambda s: "K%d-Q%d" % s)
@pytest.mark.parametrize("M", MS)
def test_empirical_equal_weights_are_the_contract_bit_for_bit(M, kq):
    K, Q = kq
    for kind in ("cont", "ties", "f32"):
        F, _, _ = quant_inputs(kind, M, K)
        got, iters = device_rows(F, EMP_LEVELS[Q], 0.0, return_iters=True)
        ref = pq.empirical_quantiles(F, EMP_LEVELS[Q])
        assert np.array_equal(bits(got), bits(ref)), (M, K, Q, kind, np.abs(got - ref).max())
        assert np.array_equal(bits(got), bits(np.quantile(F.astype(np.float64), EMP_LEVELS[Q], axis=0)))
        assert np.all(iters == 0)


@pytest.mark.parametrize("kq", KQ, ids=lambda s: "K%d-Q%d" % s)
@pytest.mark.parametrize("M", MS)
def test_empirical_weighted_equals_contract(M, kq):
    K, Q = kq
    worst = 0.0
    for kind in ("cont", "ties", "f32"):
        F, _, _ = quant_inputs(kind, M, K)
        for wkind in ("dirichlet", "half"):
            wm = quant_weights(wkind, M)
            got = device_rows(F, EMP_LEVELS[Q], 0.0, wm=wm)
            ref = pq.empirical_quantiles(F, EMP_LEVELS[Q], wm)
            dev = np.abs(got - ref).max() / np.abs(F).max()
            worst = max(worst, float(dev))
            assert np.all(np.isfinite(got)) and dev <= RTOL, (M, K, Q, kind, wkind, dev)
            if Q == 8:
                assert np.array_equal(bits(got[[0, -1]]), bits(ref[[0, -1]]))      # the levels 0 and 1 are the extreme members
    print(f"M={M} K={K} Q={Q}: largest weighted deviation / max|F| {worst:.1e}")


@pytest.mark.parametrize("kq", KQ, ids=lambda s: "K%d-Q%d" % s)
@pytest.mark.parametrize("M", MS)
def test_mixture_meets_the_residual_bound_and_the_contract(M, kq):
    K, Q = kq
    q = MIX_LEVELS[Q]
    worst_res, worst_y, most = 0.0, 0.0, 0
    for kind in ("cont", "bimodal", "f32"):
        F, V, sigma = quant_inputs(kind, M, K)
        for wm in (None, quant_weights("dirichlet", M), quant_weights("half", M)):
            for Vuse in (V, None):
                got, iters = device_rows(F, q, sigma, Vuse, wm, return_iters=True)
                res, bound = mixture_residual(got, q, F, Vuse, sigma, wm)
                worst_res = max(worst_res, float((res / bound).max()))
                most = max(most, int(iters.max()))
                assert np.all(res <= bound), (M, K, Q, kind, float((res / bound).max()))
                assert iters.min() >= 1 and iters.max() <= _lib.QUANT_MAX_ITER
                if kind != "bimodal":
                    ref = pq.mixture_quantiles(F, q, sigma, Vuse, wm)
                    dev = float((np.abs(got - ref) / np.abs(ref)).max())
                    worst_y = max(worst_y, dev)
                    assert dev <= RTOL, (M, K, Q, kind, dev)
    print(f"M={M} K={K} Q={Q}: worst residual / bound {worst_res:.2f}, worst relative deviation of y {worst_y:.1e}, most evaluations {most}")


def test_bimodal_entry_with_the_level_in_the_gap():
    F = np.array([[0.0, 0.0], [100.0, 100.0], [0.5, 0.0], [100.5, 100.0]])
    q = [0.5, 0.5 + 1e-9, 0.5 - 1e-9, 0.25]
    got, iters = device_rows(F, q, 1.0, return_iters=True)
    res, bound = mixture_residual(got, q, F, None, 1.0, None)
    print(f"gap: y {got[:, 0]}, evaluations {iters}, residual / bound {(res / bound).max():.2f}")
    assert np.all(res <= bound) and iters.max() <= _lib.QUANT_MAX_ITER and np.all(np.abs(got[:3] - 50.0) < 45.0)


@pytest.mark.parametrize("M", [2, 21, 65, 1025])
def test_the_pit_kernels_invert_the_quantiles(M):
    K, q = 67, MIX_LEVELS[8]
    for kind in ("cont", "bimodal"):
        F, V, sigma = quant_inputs(kind, M, K)
        Ft, Vt = torch.as_tensor(F).cuda(), torch.as_tensor(V).cuda()
        for wm in (None, quant_weights("half", M)):
            wt = None if wm is None else torch.as_tensor(wm).cuda()
            y = scoring.quantile_rows(Ft, q, sigma, Vt, wt)
            _, bound = mixture_residual(y.cpu().numpy(), q, F, V, sigma, wm)
            for i, qi in enumerate(q):
                yi = y[i].contiguous()
                if wm is None:
                    pit = scoring.score_rows(Ft, yi, sigma, Vt, _lib.SCORE_PIT)[2]
                else:
                    pit = scoring.score_rows_w(Ft, yi, sigma, wt, Vt, _lib.SCORE_PIT)[2]
                dev = np.abs(pit.cpu().numpy() - qi)
                assert np.all(dev <= bound[i]), (M, kind, wm is None, qi, float((dev / bound[i]).max()))


def test_isolation_and_reproducibility():
    M, K = 65, 67
    F, V, sigma = quant_inputs("cont", M, K)
    wm = quant_weights("half", M)
    for mode in ("mix", "mix_w", "emp", "emp_w"):
        q = MIX_LEVELS[8] if mode.startswith("mix") else EMP_LEVELS[8]
        kw = dict(sigma=sigma if mode.startswith("mix") else 0.0, V=V if mode.startswith("mix") else None,
                  wm=wm if mode.endswith("_w") else None)
        a, ia = device_rows(F, q, return_iters=True, **kw)
        b, ib = device_rows(F, q, return_iters=True, **kw)
        assert np.array_equal(bits(a), bits(b)) and np.array_equal(ia, ib), mode           # two calls, the same bits
        for k0, k1 in ((0, 1), (40, 41), (5, 38), (66, 67)):                               # an entry alone, another K, other blocks
            kv = dict(kw, V=None if kw["V"] is None else V[:, k0:k1])
            assert np.array_equal(bits(device_rows(F[:, k0:k1], q, **kv)), bits(a[:, k0:k1])), (mode, k0, k1)
        for i in (0, 3, 7):                                                                # a level alone, and among three
            assert np.array_equal(bits(device_rows(F, [q[i]], **kw)), bits(a[i:i + 1])), (mode, i)
        assert np.array_equal(bits(device_rows(F, [q[6], q[1], q[4]], **kw)), bits(a[[6, 1, 4]])), mode
        q16 = list(q) + [0.1, 0.2, 0.3, 0.4, 0.6, 0.7, 0.8, 0.9]                           # more levels than one launch holds
        c, ic = device_rows(F, q16, return_iters=True, **kw)
        assert np.array_equal(bits(c[:8]), bits(a)) and np.all(ic >= ia) and ic.max() <= _lib.QUANT_MAX_ITER, mode
        # a NaN f, and s^2 <= 0 in mixture mode, make that entry NaN and no other; what a member without weight holds plays no part
        G, W = F.copy(), V.copy()
        G[4, 20] = np.nan
        G[1, 7] = np.nan                                                                   # member 1 has no weight in 'half'
        W[6, 41] = -sigma ** 2
        kv = dict(kw, V=None if kw["V"] is None else W)
        d, idd = device_rows(G, q, return_iters=True, **kv)
        nan = [20] + ([41] if mode.startswith("mix") else []) + ([] if mode.endswith("_w") else [7])
        keep = np.setdiff1d(np.arange(K), nan)
        assert np.all(np.isnan(d[:, nan])) and np.all(idd[nan] == 0), mode
        assert np.array_equal(bits(d[:, keep]), bits(a[:, keep])) and np.array_equal(idd[keep], ia[keep]), mode
    for bad in (-1e-3, float("nan")):
        w = wm.copy()
        w[2] = bad
        assert np.all(np.isnan(device_rows(F, [0.5], sigma, V, w))) and np.all(np.isnan(device_rows(F, [0.5], 0.0, None, w)))


@pytest.mark.parametrize("M", [8192, 8193, 16384])
def test_empirical_mode_at_the_largest_member_counts(M):
    """8192 is the last count whose sort keeps the member indices in LDS, 8193 the first that keeps them in the workspace."""
    F, _, _ = quant_inputs("ties", M, 3)
    q = EMP_LEVELS[8]
    assert np.array_equal(bits(device_rows(F, q, 0.0)), bits(np.quantile(F, q, axis=0)))
    wm = quant_weights("half", M)
    got, ref = device_rows(F, q, 0.0, wm=wm), pq.empirical_quantiles(F, q, wm)
    dev = np.abs(got - ref).max() / np.abs(F).max()
    print(f"M={M}: largest weighted deviation / max|F| {dev:.1e}")
    assert dev <= RTOL and np.array_equal(bits(got[[0, -1]]), bits(ref[[0, -1]]))


def test_refusals_on_the_device_path():
    F = torch.zeros(4, 3, dtype=torch.float64).cuda()
    for kw in (dict(q=[0.0], noise=0.1), dict(q=[1.5], noise=0.0), dict(q=[0.5] * 17, noise=0.1), dict(q=[0.5], noise=-1.0)):
        with pytest.raises(ValueError):
            scoring.quantile_rows(F, kw["q"], kw["noise"])
    out = scoring.pred_quantiles(np.arange(12.0).reshape(4, 3, 1), [0.0, 0.5, 1.0], 0.0)
    assert out.shape == (3, 3, 1) and np.array_equal(out[:, :, 0], np.quantile(np.arange(12.0).reshape(4, 3), [0.0, 0.5, 1.0], axis=0))


# ------------------------------------------------------------------------------------------ the solver surface
@pytest.fixture(scope="module")
def fit():
    from quinn_amd.nns.mlp import MLP
    from quinn_amd.solvers.nn_mcmc import NN_MCMC
    rs = np.random.RandomState(0)
    x = rs.rand(40, 1) * 6 - 3
    y = np.sin(x) + 0.1 * rs.randn(40, 1)
    torch.manual_seed(0)
    uq = NN_MCMC(MLP(1, 1, (16,), activ='tanh'), verbose=False)
    C = 4
    ini = np.stack([np.random.RandomState(100 + c).rand(uq.pdim) for c in range(C)])
    uq.fit(x, y, zflag=False, datanoise=0.2, nmcmc=300, param_ini=ini, sampler='amcmc',
           sampler_params={'gamma': 0.1, 't0': 50, 'tadapt': 100}, seeds=list(range(C)), engine='device')
    return uq, x, y


def test_solver_quantiles(fit):
    uq, x, y = fit
    ens = dict(nsam=60, nburn=150, chain='all')
    q = [0.0, 0.05, 0.25, 0.5, 0.75, 0.95, 1.0]
    members = uq.predict_ens(x, nens=60, nburn=150, chain='all')
    epi = uq.predict_quantiles(x, q=q, noise=0, **ens)
    assert epi.shape == (7, 40, 1) and np.array_equal(bits(epi), bits(np.quantile(members, q, axis=0)))
    assert np.array_equal(bits(epi), bits(uq.predict_quantiles(x, q=q, noise=False, **ens)))
    lo, mid, hi = uq.predict_interval(x, level=0.9, **ens)
    assert lo.shape == (40, 1) and np.all(lo <= mid) and np.all(mid <= hi)
    assert np.all(hi - lo > epi[5] - epi[1])                            # the data noise widens the epistemic band
    s = uq.score(x, y, crps=False, **ens)
    band = scoring.interval_summary(lo, hi, y, 0.9)
    assert band["coverage"] == s["coverage"][0.9] and band["width"] > 0 and band["interval_score"] >= band["width"]
    levels = (0.5 * (1.0 - 0.9), 0.5, 0.5 * (1.0 + 0.9))                # as predict_interval forms them
    full = uq.predict_quantiles(x, q=levels, **ens)
    assert np.array_equal(bits(full[[0, 2]]), bits(np.stack([lo, hi]))) and np.array_equal(bits(full[1]), bits(mid))
    small = uq.predict_quantiles(x, q=levels, max_bytes=7 * 60 * 8, **ens)        # seven rows per chunk
    assert np.array_equal(bits(small), bits(full))
    assert np.array_equal(bits(uq.predict_quantiles(x, q=q, noise=0, max_bytes=1, **ens)), bits(epi))
    # the stacked band: the members of the chains that carry no weight play no part
    wm = np.zeros(60)
    wm[:15] = 1.0 / 15
    a = uq.predict_quantiles(x, member_weights=wm, **ens)
    W = uq._ens_weights_ordered(60, nburn=150, chain='all')[:15]
    F = uq._predict_batch_dev(W, x).reshape(15, -1).contiguous()
    b = scoring.quantile_rows(F, [0.05, 0.5, 0.95], 0.2).cpu().numpy().reshape(3, 40, 1)
    assert np.allclose(a, b, rtol=1e-12, atol=1e-13)
    with pytest.raises(ValueError):
        uq.predict_quantiles(x, member_weights=wm[:10], **ens)


def test_glm_quantiles_of_one_member():
    from quinn_amd.nns.mlp import MLP
    from quinn_amd.solvers.nn_laplace import NN_Laplace
    rs = np.random.RandomState(1)
    x = rs.rand(30, 1) * 4 - 2
    y = np.sin(x) + 0.1 * rs.randn(30, 1)
    torch.manual_seed(1)
    uq = NN_Laplace(MLP(1, 1, (8,), biasorno=True, activ='tanh').double(), la_type='ggn_diag', nens=1, dfrac=1.0, datanoise=0.1,
                    verbose=False)
    uq.fit(x, y, val=[x, y], lrate=0.01, batch_size=10, nepochs=50, freq_out=1000)
    q = [0.05, 0.5, 0.95]
    z = pq.inv_normal_cdf(q)
    for noise in (False, True):
        mean, var, _ = uq.predict_glm(x, msc=1, noise=noise)
        got = uq.predict_glm_quantiles(x, q, noise=noise)
        ref = mean[None] + np.sqrt(var)[None] * z[:, None, None]
        assert got.shape == (3, 30, 1) and np.allclose(got, ref, rtol=1e-12, atol=1e-13), np.abs(got - ref).max()
