"""GPU: qn_chain_stats (csrc/qn_diag.hip) against the numpy restatement of tests/test_chain_diag_cpu.py over every launch
regime, its numerical and NaN guarantees, and the NN_MCMC surface built on it (fit(diagnostics=True), diagnose,
predict_ens(chain='all'), predict_MAP(chain='best')).

Bars (float64 sums of at most ~1e4 terms carry ~1e4 * 2^-53 = 1e-12; two to three orders are left for summation order):
means 1e-10 and the two scatter rows 1e-9, relative to the largest magnitude of the row stats[c, r, :]."""
import numpy as np
import pytest
import torch

from quinn_amd.mcmc import diagnostics as diag
from quinn_amd.nns.mlp import MLP
from quinn_amd.solvers.nn_mcmc import NN_MCMC
from test_chain_diag_cpu import ar1, assert_same_diagnostics, diagnostics_np, stats_np

pytestmark = pytest.mark.gpu

SHAPES = [(1, 50, 1), (3, 1001, 7), (2, 4097, 321), (64, 300, 1), (5, 777, 1025), (64, 2001, 513)]
BARS = (1e-10, 1e-10, 1e-9, 1e-9, 1e-9, 1e-9)


def assert_stats_close(got, ref, rows=range(6), what=""):
    for r in rows:
        scale = np.max(np.abs(ref[:, r]), axis=1, keepdims=True)
        err = np.max(np.abs(got[:, r] - ref[:, r]) / scale)
        print(f"{what} stats row {r}: max error / row max = {err:.3e} (bar {BARS[r]:.0e})")
        assert err <= BARS[r], (what, r, err)


def dev_stats(x, nburn):
    return diag.chain_stats(torch.as_tensor(x).cuda(), nburn).cpu().numpy()


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_equals_numpy(shape, dtype):
    C, T, K = shape
    x = (ar1(7, C, T, K, rho=0.7) * 1.5 + 0.25).astype(dtype)
    for nburn in (0, 1, T // 3 | 1):
        got = dev_stats(x, nburn)
        assert got.shape == (C, 6, K)
        assert_stats_close(got, stats_np(x, nburn), what=f"{shape} {np.dtype(dtype).name} nburn={nburn}")
        t0, nbatch, blen = diag.batch_plan(T, nburn)
        assert_same_diagnostics(diag.combine(got, nbatch, blen, t0), diagnostics_np(x, nburn), 1e-9)


def test_host_array_is_uploaded_in_pieces():
    x = ar1(2, 5, 400, 33, rho=0.5)
    whole = dev_stats(x, 11)
    pieces = diag.chain_stats(x, 11, max_upload_bytes=2 * 400 * 33 * 8)        # two chains per piece, then one
    assert pieces.is_cuda and np.array_equal(pieces.cpu().numpy(), whole)
    assert np.array_equal(diag.chain_stats(x[3], 11).cpu().numpy(), whole[3:4])            # a single 2-D chain is C = 1


@pytest.mark.parametrize("shape", [(3, 1001, 7), (5, 777, 1025), (64, 300, 1)], ids=lambda s: "x".join(map(str, s)))
def test_large_offset_costs_no_digits(shape):
    """std 1 on top of 1e6: the naive sum(x^2) - n mean^2 is off by ~5e-3 here, a shifted sum by ~1e-14.  Against a long-double
    evaluation the kernel's arithmetic (restated in numpy) is within 6e-14 on every row; numpy's own float64 batch means of values
    near 1e6 leave 1.4e-10 .. 3.9e-10 on the batch-mean scatter (rows 4, 5), which is what this comparison then shows."""
    x = ar1(11, *shape, rho=0.7) + 1e6
    assert_stats_close(dev_stats(x, 0), stats_np(x, 0), rows=(2, 3, 4, 5), what=f"{shape} offset 1e6")


def test_two_calls_same_bits_and_chain_subsets():
    x = torch.as_tensor(ar1(5, 6, 901, 130, rho=0.8)).cuda()
    a, b = diag.chain_stats(x, 100), diag.chain_stats(x, 100)
    assert torch.equal(a, b)
    assert torch.equal(diag.chain_stats(x[2:5].contiguous(), 100), a[2:5])    # no dependence on C or on the launch it implies


def test_nan_stays_in_its_half():
    C, T, K = 4, 601, 70
    x = ar1(9, C, T, K, rho=0.6)
    clean = dev_stats(x, 50)
    t0, nbatch, blen = diag.batch_plan(T, 50)
    n = nbatch * blen
    for (c, t, k), bad in [((2, t0 + 5, 3), np.nan), ((0, t0 + n + 2 * blen + 1, 69), np.nan), ((3, T - 1, 0), np.inf),
                           ((1, t0, 10), np.nan), ((1, t0 + n, 11), -np.inf)]:
        y = x.copy()
        y[c, t, k] = bad
        got = dev_stats(y, 50)
        h = int(t >= t0 + n)
        hit = np.zeros(got.shape, dtype=bool)
        hit[c, [h, 2 + h, 4 + h], k] = True
        assert not np.isfinite(got[hit]).any(), (c, t, k)
        if np.isnan(bad):
            assert np.isnan(got[hit]).all(), (c, t, k)
        assert np.array_equal(got[~hit], clean[~hit]), (c, t, k)
    y = x.copy()
    y[1, t0 - 1, 5] = np.nan                                  # before the window: not read at all
    assert np.array_equal(dev_stats(y, 50), clean)


def test_refusals():
    x = torch.zeros(2, 100, 4, dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError):
        diag.chain_stats(x, 95)
    with pytest.raises(ValueError):
        diag.chain_stats(x.transpose(1, 2), 0)                # not contiguous: refused, never copied silently
    with pytest.raises(ValueError):
        diag.chain_stats(x.half(), 0)


# ---- the NN_MCMC surface ----------------------------------------------------------------------------------------------------
def _problem(N=48, seed=0):
    rs = np.random.RandomState(seed)
    x = rs.rand(N, 1) * 6 - 3
    return x, np.sin(x) + 0.1 * rs.randn(N, 1)


def _fit(engine, nmcmc=600, C=4, **kw):
    x, y = _problem()
    torch.manual_seed(0)
    uq = NN_MCMC(MLP(1, 1, (8, 8), activ='tanh'), verbose=False)
    ini = np.stack([np.random.RandomState(100 + c).rand(uq.pdim) for c in range(C)])
    uq.fit(x, y, zflag=False, datanoise=0.2, nmcmc=nmcmc, param_ini=ini, sampler='amcmc',
           sampler_params={'gamma': 0.1, 't0': 50, 'tadapt': 100}, seeds=list(range(C)), engine=engine, **kw)
    return uq


@pytest.fixture(scope="module")
def fitted():
    return _fit('device', diagnostics=True, gather_chain='none')


def test_fit_diagnostics_device_engine(fitted):
    uq = fitted
    again = _fit('device')                                    # device chains are reproducible per seed
    assert again.diagnostics is None
    assert np.array_equal(again.samples, uq.samples)
    assert_same_diagnostics(uq.diagnostics['params'], diagnostics_np(again.samples, 300), 1e-9)
    lp = uq.diagnostics['logpost']
    assert lp['rhat'].shape == (1,) and lp['ess'].shape == (1,)
    assert_same_diagnostics(lp, diagnostics_np(again.mcmc_results['logpost'][:, :, None], 300), 1e-9)
    assert uq.diagnostics['params']['rhat'].shape == (uq.pdim,)


def test_fit_diagnostics_host_engine():
    uq = _fit('host', nmcmc=300, diagnostics=True, diag_nburn=101)
    assert_same_diagnostics(uq.diagnostics['params'], diagnostics_np(uq.samples, 101), 1e-9)
    assert_same_diagnostics(uq.diagnostics['logpost'], diagnostics_np(uq.mcmc_results['logpost'][:, :, None], 101), 1e-9)
    assert uq.diagnostics['logpost']['rhat'].shape == (1,)


def test_diagnose_function_space(fitted):
    uq = fitted
    xg = np.linspace(-3, 3, 9)[:, None]
    d = uq.diagnose(xg, nburn=200, nens=40)
    assert_same_diagnostics(d['params'], diagnostics_np(uq.samples, 200), 1e-9)
    byhand = np.stack([uq.predict_ens(xg, nens=40, nburn=200, chain=c) for c in range(4)])      # [C, nens, N, o]
    ref = diagnostics_np(byhand.reshape(4, 40, 9), 0)
    for k in ('rhat', 'ess', 'mean', 'var'):
        ref[k] = ref[k].reshape(9, 1)
    assert d['pred']['rhat'].shape == (9, 1)
    assert_same_diagnostics(d['pred'], ref, 1e-9)
    assert 'pred' not in uq.diagnose(nburn=200)


def test_predict_ens_pools_chains(fitted):
    uq = fitted
    xg = np.linspace(-3, 3, 7)[:, None]
    pooled = uq.predict_ens(xg, nens=10, nburn=100, chain='all')
    parts = [uq.predict_ens(xg, nens=cnt, nburn=100, chain=c) for c, cnt in enumerate([3, 3, 2, 2])]
    assert pooled.shape == (10, 7, 1) and np.array_equal(pooled, np.concatenate(parts))
    # chain=<int>: today's rows, today's forward
    rows = [100 + j * int((601 - 100) / 10) for j in range(10)]
    for c in (0, 2):
        assert np.array_equal(uq.predict_ens(xg, nens=10, nburn=100, chain=c), uq._predict_batch(uq.samples[c][rows, :], xg))
    assert np.array_equal(uq.predict_ens(xg, nens=10, nburn=100), uq.predict_ens(xg, nens=10, nburn=100, chain=0))
    with pytest.raises(ValueError):
        uq.predict_ens(xg, chain='every')
    m_all = uq.predict_mom_sample(xg, msc=1, nsam=10, nburn=100, chain='all')
    assert np.allclose(m_all[0], pooled.mean(axis=0), rtol=1e-12, atol=1e-14)
    assert np.allclose(m_all[1], pooled.var(axis=0, ddof=1), rtol=1e-10, atol=1e-14)
    m0 = uq.predict_mom_sample(xg, msc=0, nsam=10, nburn=100)
    assert np.allclose(m0[0], uq.predict_ens(xg, nens=10, nburn=100).mean(axis=0), rtol=1e-12, atol=1e-14)


def test_predict_map_best_chain(fitted):
    uq = fitted
    xg = np.linspace(-3, 3, 5)[:, None]
    best = int(np.argmax(uq.mcmc_results['maxpost']))
    assert np.array_equal(uq.predict_MAP(xg), uq.predict_sample(xg, uq.cmode[0]))
    assert np.array_equal(uq.predict_MAP(xg, chain='best'), uq.predict_sample(xg, uq.cmode[best]))
