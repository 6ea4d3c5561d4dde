"""GPU: `qn_rank_diag` (csrc/qn_rank.hip) against its numpy contract (`quinn_amd/mcmc/rankdiag.py`), its isolation and
reproducibility properties, and the solver surface.

Tolerance rtol = 1e-9 on all six rows: sums of at most 16384 float64 terms of order 1 carry about S eps ~ 4e-12, the two
inverse normal CDFs (both Wichura's AS241) agree to a few ulp, and tau >= 1 / log10(S) ~ 0.24 bounds the cancellation in
tau: about two orders of margin.  Every comparison prints the largest relative deviation it saw before it asserts."""
import numpy as np
import pytest
import torch

from quinn_amd import _lib
from quinn_amd.mcmc import rankdiag as rd
from test_rank_diag_cpu import rank_inputs

pytestmark = pytest.mark.gpu

SHAPES = [(1, 4, 1), (3, 5, 5), (7, 9, 67), (64, 128, 3), (1, 8192, 2)]
KINDS = ["cont", "ties", "offset", "f32", "window"]
RTOL = 1e-9


def device_rows(x, t0, nh, stride):
    t = torch.as_tensor(np.ascontiguousarray(x)).cuda()
    return rd._device_rows(t, t0, nh, stride).cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "C%d-nh%d-K%d" % s)
def test_device_equals_contract(shape, kind):
    C, nh, K = shape
    x, t0, stride = rank_inputs(kind, C, nh, K)
    ref = rd.rank_rows(x, t0, nh, stride)
    got = device_rows(x, t0, nh, stride)
    # NaN where the contract says NaN (an indicator without within-sequence variance at the smallest S), and only there
    assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.isfinite(ref).sum() >= ref.size - 1 and not np.isinf(got).any()
    dev = np.where(np.isnan(ref), 0.0, np.abs(got - ref) / np.abs(ref))
    print(f"{shape} {kind}: largest relative deviation per row " + " ".join(f"{d:.1e}" for d in dev.max(axis=1)))
    assert np.all(dev <= RTOL), dev.max(axis=1)


def test_scaling_by_four_keeps_the_bits():
    for kind in ("cont", "ties"):
        x, t0, stride = rank_inputs(kind, 7, 9, 67)
        a, b = device_rows(x, t0, 9, stride), device_rows(4.0 * x, t0, 9, stride)
        assert np.array_equal(bits(a[:4]), bits(b[:4]))


def test_isolation_and_reproducibility():
    C, nh, K = 7, 9, 67
    x, _, _ = rank_inputs("cont", C, nh, K)
    a = device_rows(x, 0, nh, 1)
    assert np.array_equal(bits(a), bits(device_rows(x, 0, nh, 1)))                     # two calls, the same bits
    y = x.copy()
    y[3, 11, 20] = np.nan
    y[:, :, 41] = -2.5
    b = device_rows(y, 0, nh, 1)
    keep = np.setdiff1d(np.arange(K), [20, 41])
    assert np.all(np.isnan(b[:, 20])) and np.all(np.isnan(b[:, 41]))
    assert np.array_equal(bits(b[:, keep]), bits(a[:, keep]))
    for k0, k1 in ((0, 1), (5, 38), (60, 67)):                                         # columns copied out: another K, other blocks
        assert np.array_equal(bits(device_rows(x[:, :, k0:k1], 0, nh, 1)), bits(a[:, k0:k1])), (k0, k1)
    # rows around the window do not matter: a longer chain, the same rows selected
    z = np.concatenate([np.full((C, 3, K), 7.0), x, np.full((C, 2, K), -7.0)], axis=1)
    assert np.array_equal(bits(device_rows(z, 3, nh, 1)), bits(a))


def test_chunked_host_upload_equals_the_call_in_place():
    x, _, _ = rank_inputs("cont", 3, 5, 5)
    t = torch.as_tensor(x).cuda()
    a = rd.rank_stats(t)
    b = rd.rank_stats(x, max_bytes=3 * 30 * 8 * 2)                                     # two entries per chunk
    c = rd.rank_stats(t, max_bytes=1)
    for k in rd.KEYS + ("rhat_rank",):
        assert np.array_equal(bits(a[k]), bits(b[k])) and np.array_equal(bits(a[k]), bits(c[k])), k
    assert (a["n_draws"], a["nh"], a["stride"], a["t0"]) == (30, 5, 1, 0)
    ref = rd.rank_stats_host(x)
    assert np.allclose(a["ess_bulk"], ref["ess_bulk"], rtol=RTOL)


def test_too_many_draws_is_refused_with_null_pointers():
    L = _lib.lib()
    rc = L.qn_rank_diag(None, _lib.QN_F64, 1, 100000, 3, 0, _lib.RANK_MAX_S // 2 + 1, 1, None, None, 0, None)
    assert rc == _lib.CONSTANTS["QN_EINVAL"] and b"at most" in L.qn_last_error()


def _fit(nmcmc=300, C=4, **kw):
    from quinn_amd.nns.mlp import MLP
    from quinn_amd.solvers.nn_mcmc import NN_MCMC
    rs = np.random.RandomState(0)
    x = rs.rand(40, 1) * 6 - 3
    y = np.sin(x) + 0.1 * rs.randn(40, 1)
    torch.manual_seed(0)
    uq = NN_MCMC(MLP(1, 1, (8, 8), activ='tanh'), verbose=False)
    ini = np.stack([np.random.RandomState(100 + c).rand(uq.pdim) for c in range(C)])
    uq.fit(x, y, zflag=False, datanoise=0.2, nmcmc=nmcmc, param_ini=ini, sampler='amcmc',
           sampler_params={'gamma': 0.1, 't0': 50, 'tadapt': 100}, seeds=list(range(C)), engine='device', **kw)
    return uq, x


def test_solver_surface():
    new = {"rhat_bulk", "rhat_tail", "rhat_rank", "ess_bulk", "ess_tail", "ess_mean", "mcse_mean", "rank_n_draws", "rank_nh",
           "rank_stride", "rank_t0"}
    ranked, _ = _fit(diagnostics='rank', gather_chain='none')          # from the engine's own tensors: nothing was gathered
    uq, x = _fit(diagnostics=True)
    for k in ("params", "logpost"):
        assert not set(uq.diagnostics[k]) & new and set(ranked.diagnostics[k]) == set(uq.diagnostics[k]) | new, k
        for name in set(uq.diagnostics[k]):                            # what diagnostics=True computes is what it was
            assert np.array_equal(np.asarray(uq.diagnostics[k][name]), np.asarray(ranked.diagnostics[k][name]), equal_nan=True), (k, name)
    d = ranked.diagnostics
    assert d["params"]["ess_bulk"].shape == (uq.pdim,) and d["logpost"]["rhat_rank"].shape == (1,)
    T = np.asarray(uq.samples).shape[1]
    ref = rd.rank_stats(np.asarray(uq.samples), nburn=300 // 2)
    lref = rd.rank_stats(np.asarray(uq.mcmc_results['logpost'])[:, :, None], nburn=300 // 2)
    for k in rd.KEYS:
        assert np.array_equal(bits(d["params"][k]), bits(ref[k])), k
        assert np.array_equal(bits(d["logpost"][k]), bits(lref[k])), k
    assert d["params"]["rank_n_draws"] == ref["n_draws"] == 8 * ref["nh"] and ref["t0"] + (2 * ref["nh"] - 1) * ref["stride"] == T - 1
    plain = uq.diagnose(x, nburn=150, nens=20)
    out = uq.diagnose(x, nburn=150, nens=20, rank=True)
    assert set(plain["pred"]) | new == set(out["pred"]) and not set(plain["pred"]) & new
    assert out["pred"]["ess_bulk"].shape == (40, 1) and out["params"]["rhat_tail"].shape == (uq.pdim,)
