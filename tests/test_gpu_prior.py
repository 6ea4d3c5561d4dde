"""GPU: the Gaussian weight prior of `NN_MCMC` (qn_prior_fold behind every forward / gradient call of the device engines).  The
kernel is checked against `prior.fold` (gradient bit for bit, sum of squares to the bound of any summation order, run-to-run
and launch-split reproducibility, non-finite rows; the three fold entry points, one kernel, agree in every bit), every engine's stored trace against the host formula with the prior, one HMC
step against the numpy leapfrog, the host gradient against central differences, the samplers in distribution on a posterior
that exists only because of the prior, and the default (no prior), graph and group paths for bit-identity."""
import math

import numpy as np
import pytest
import torch

from oracle import mlp_ref
from quinn_amd import _lib
from quinn_amd.mcmc import prior as pr
from quinn_amd.mcmc import sgmcmc as sg
from quinn_amd.mcmc.device_amcmc import DeviceAMCMC
from quinn_amd.mcmc.device_hmc import DeviceHMC
from quinn_amd.mcmc.device_mala import DeviceMALA
from quinn_amd.mcmc.device_sgmcmc import DeviceSGHMC, DeviceSGLD
from quinn_amd.ops import BatchedMLP, MLPArch

pytestmark = pytest.mark.gpu

KEYS = ('chain', 'logpost', 'alphas', 'accrate', 'mapparams', 'maxpost')
LAM, C0 = 0.37, -1.25


def _problem(seed=0, N=48, d=1):
    rs = np.random.RandomState(seed)
    x = rs.rand(N, d) * 6 - 3
    y = np.sin(x).sum(axis=1, keepdims=True) + 0.1 * rs.randn(N, 1)
    return x, y


def _fold(W, grad=None, sse=None, stride=1, lam=LAM, c0=C0):
    """qn_prior_fold through the C ABI on copies of grad / sse (W, grad, sse: numpy) -> (grad', sse') numpy, None for None."""
    dev = "cuda"
    Wt = torch.as_tensor(np.ascontiguousarray(W), device=dev)
    gt = None if grad is None else torch.as_tensor(np.ascontiguousarray(grad), device=dev)
    st = None if sse is None else torch.as_tensor(np.ascontiguousarray(sse), device=dev)
    ptr = lambda t: None if t is None else t.data_ptr()
    gdt = _lib.QN_F32 if gt is not None and gt.dtype == torch.float32 else _lib.QN_F64
    C, p = Wt.shape
    _lib.check(_lib.lib().qn_prior_fold(Wt.data_ptr(), lam, c0, ptr(gt), gdt, ptr(st), stride, C, p, None), "qn_prior_fold")
    torch.cuda.synchronize()
    assert np.array_equal(Wt.cpu().numpy(), W, equal_nan=True)               # the weights are read only
    return (None if gt is None else gt.cpu().numpy()), (None if st is None else st.cpu().numpy())


def _sse_ref_and_tol(w, sse0):
    """Reference and bound for one chain: ref with math.fsum; |got - ref| <= p 2^-52 (lam sum w^2) + 2^-52 |ref| --
    the worst case of any summation order of non-negative terms, plus the two final additions."""
    ssq = math.fsum(float(v) * float(v) for v in w)
    ref = float(sse0) + (LAM * ssq + C0)
    return ref, len(w) * 2.0 ** -52 * (LAM * ssq) + 2.0 ** -52 * abs(ref)


@pytest.mark.parametrize("p", [1, 7, 4099])
def test_kernel_equals_the_numpy_fold(p):
    """C = 3 rows of odd length (8-byte aligned only), shorter than one access pair, longer than one pass of a workgroup."""
    rs = np.random.RandomState(p)
    C = 3
    W = rs.randn(C, p)
    g64 = 3.0 * rs.randn(C, p)
    sse1 = 10.0 + 40.0 * rs.rand(C)                                          # (an SSE is positive)
    sse3 = 10.0 + 40.0 * rs.rand(C, 3)
    for g in (g64, g64.astype(np.float32)):
        want_g, _ = pr.fold(W, LAM, C0, grad=g)
        got_g, none = _fold(W, grad=g)                                       # sse NULL
        assert none is None and got_g.dtype == g.dtype
        np.testing.assert_allclose(got_g, want_g, rtol=0, atol=0)
        got_g2, got_s = _fold(W, grad=g, sse=sse1)                           # both
        np.testing.assert_allclose(got_g2, want_g, rtol=0, atol=0)
        only_s = _fold(W, sse=sse1)[1]                                       # grad NULL: the same sum, another grid
        assert np.array_equal(got_s, only_s)
        for c in range(C):
            ref, tol = _sse_ref_and_tol(W[c], sse1[c])
            print(p, g.dtype, c, "sse", got_s[c], "ref", ref, "err", abs(got_s[c] - ref), "tol", tol)
            assert abs(got_s[c] - ref) <= tol
        # two calls give equal bits
        again_g, again_s = _fold(W, grad=g, sse=sse1)
        assert np.array_equal(again_g, got_g2) and np.array_equal(again_s, got_s)
    # sse_stride = 3: column 0 receives the term, the other columns are unchanged bit for bit
    got3 = _fold(W, sse=sse3, stride=3)[1]
    assert np.array_equal(got3[:, 1:], sse3[:, 1:])
    for c in range(C):
        ref, tol = _sse_ref_and_tol(W[c], sse3[c, 0])
        assert abs(got3[c, 0] - ref) <= tol
    assert np.array_equal(got3[:, 0], _fold(W, sse=np.ascontiguousarray(sse3[:, 0]))[1])


@pytest.mark.parametrize("p", [1, 7, 4099])
def test_a_chain_does_not_depend_on_the_launch_it_is_in(p):
    rs = np.random.RandomState(100 + p)
    W, g, sse = rs.randn(5, p), rs.randn(5, p), 5.0 + rs.rand(5)
    for gg in (g, g.astype(np.float32)):
        whole = _fold(W, grad=gg, sse=sse)
        a = _fold(W[:2], grad=gg[:2], sse=sse[:2])
        b = _fold(W[2:], grad=gg[2:], sse=sse[2:])
        assert np.array_equal(np.concatenate([a[0], b[0]]), whole[0])
        assert np.array_equal(np.concatenate([a[1], b[1]]), whole[1])


@pytest.mark.parametrize("p", [7, 4099])
def test_non_finite_weights_stay_in_their_chain(p):
    rs = np.random.RandomState(200 + p)
    W, g, sse = rs.randn(3, p), rs.randn(3, p), 5.0 + rs.rand(3)
    clean_g, clean_s = _fold(W, grad=g, sse=sse)
    for bad, check in ((np.inf, lambda v: v == np.inf), (-np.inf, lambda v: v == np.inf), (np.nan, np.isnan)):
        Wb = W.copy()
        Wb[1, p // 2] = bad
        got_g, got_s = _fold(Wb, grad=g, sse=sse)
        assert check(got_s[1]), (bad, got_s)
        assert np.array_equal(got_s[[0, 2]], clean_s[[0, 2]]) and np.array_equal(got_g[[0, 2]], clean_g[[0, 2]])
        mask = np.ones(p, dtype=bool)
        mask[p // 2] = False
        assert np.array_equal(got_g[1, mask], clean_g[1, mask])


# ------------------------------------------------------------------- one fold kernel behind three entry points
def _three_folds(W, grad=None, sse=None, stride=1):
    """The scalar prior (LAM, C0) through qn_prior_fold, through qn_prior_fold_g as one group [0, p) with lam[c, 0] = LAM,
    c0[c] = C0, and through qn_noise_fold with that group, kappa = 1 and d0 = 0 -> three (grad', sse') pairs, numpy."""
    L = _lib.lib()
    C, p = W.shape
    dev = lambda a: None if a is None else torch.as_tensor(np.ascontiguousarray(a), device="cuda")
    ptr = lambda t: None if t is None else t.data_ptr()
    Wt, lam, c0, seg = dev(W), dev(np.full((C, 1), LAM)), dev(np.full(C, C0)), dev(np.array([0, p], dtype=np.int64))
    kappa, d0 = dev(np.ones(C)), dev(np.zeros(C))
    gdt = _lib.QN_F32 if grad is not None and grad.dtype == np.float32 else _lib.QN_F64
    out = []
    for name in ("qn_prior_fold", "qn_prior_fold_g", "qn_noise_fold"):
        gt, st = dev(grad), dev(sse)
        rest = (ptr(gt), gdt, ptr(st), stride, C, p, None)
        group = (lam.data_ptr(), c0.data_ptr(), seg.data_ptr(), 1)
        args = {"qn_prior_fold": (LAM, C0), "qn_prior_fold_g": group, "qn_noise_fold": (kappa.data_ptr(), d0.data_ptr()) + group}
        _lib.check(getattr(L, name)(Wt.data_ptr(), *args[name], *rest), name)
        torch.cuda.synchronize()
        out.append((None if gt is None else gt.cpu().numpy(), None if st is None else st.cpu().numpy()))
    return out


def _same_bits(a, b):
    return (a is None and b is None) or (a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8)))


@pytest.mark.parametrize("p", [1, 7, 1024, 1025, 4099])
def test_the_three_entry_points_are_one_fold_bit_for_bit(p):
    """C = 3; p = 1024 / 1025 straddle the chunk at which a chain goes from one workgroup to two, 4099 gives five with a ragged
    tail.  Gradient (float64, float32) AND SSE of the three entry points agree in every bit, for sse_stride 1 and 3, and the SSE
    is the same with and without a gradient (another grid).  The SSE is positive: kappa = 1, d0 = 0 alters no bit of it."""
    rs = np.random.RandomState(300 + p)
    C = 3
    W, g64 = rs.randn(C, p), 3.0 * rs.randn(C, p)
    for stride in (1, 3):
        sse = 10.0 + 40.0 * rs.rand(C * stride)
        assert C0 + sse.min() > 0.0
        alone = _three_folds(W, sse=sse, stride=stride)                       # grad NULL: one workgroup per chain
        for g in (g64, g64.astype(np.float32)):
            both = _three_folds(W, grad=g, sse=sse, stride=stride)
            only_g = _three_folds(W, grad=g, stride=stride)                   # sse NULL
            for k in (1, 2):
                assert _same_bits(both[k][0], both[0][0]) and _same_bits(both[k][1], both[0][1]), (stride, g.dtype, k)
                assert _same_bits(only_g[k][0], both[0][0]) and only_g[k][1] is None
                assert _same_bits(alone[k][1], both[0][1]) and alone[k][0] is None
            assert _same_bits(only_g[0][0], both[0][0]) and _same_bits(alone[0][1], both[0][1])
            assert both[0][0].dtype == g.dtype and np.all(both[0][1].reshape(C, stride)[:, 0] > 0.0)
            assert np.array_equal(both[0][1].reshape(C, stride)[:, 1:], sse.reshape(C, stride)[:, 1:])


@pytest.mark.parametrize("p", [1, 7, 1024, 1025, 4099])
def test_a_nan_row_leaves_the_other_rows_of_every_entry_point_as_a_launch_without_it(p):
    rs = np.random.RandomState(400 + p)
    W, g, sse = rs.randn(3, p), rs.randn(3, p), 5.0 + rs.rand(3)
    W[1, p // 2] = np.nan
    keep = [0, 2]
    for gg in (g, g.astype(np.float32)):
        with_row = _three_folds(W, grad=gg, sse=sse)
        without = _three_folds(W[keep], grad=gg[keep], sse=sse[keep])
        for (got_g, got_s), (want_g, want_s) in zip(with_row, without):
            assert np.isnan(got_s[1]) and np.isnan(got_g[1, p // 2])
            assert _same_bits(np.ascontiguousarray(got_g[keep]), want_g) and _same_bits(np.ascontiguousarray(got_s[keep]), want_s)


# ---------------------------------------------------------------------------------------------- engines
PS = 0.8
ENGINES = {
    'amcmc': ('amcmc', {'gamma': 0.1}),
    'hmc': ('hmc', {'epsilon': 0.002, 'L': 2}),
    'mala': ('mala', {'epsilon': 0.003}),
    'hmc_adapt': ('hmc', {'epsilon': 0.002, 'L': 2, 'adapt': 10}),
    'hmc_ladder': ('hmc', {'epsilon': 0.002, 'L': 2, 'ladder': 2, 'beta_min': 0.3}),
    'sgld_full': ('sgld', {'eta': 2e-6, 'batch': None}),
    'sghmc_mini': ('sghmc', {'eta': 2e-6, 'alpha': 0.1, 'batch': 16, 'thin': 2}),
}


def _solver(hidden=(16, 16), d=1):
    from quinn_amd.nns.mlp import MLP
    from quinn_amd.solvers.nn_mcmc import NN_MCMC
    torch.manual_seed(0)
    return NN_MCMC(MLP(d, 1, hidden, activ="tanh"), verbose=False, kernels="float64")


@pytest.mark.parametrize("name", list(ENGINES))
def test_stored_trace_is_the_log_posterior_with_the_prior(name):
    sampler, params = ENGINES[name]
    x, y = _problem(seed=2, N=64)
    # (the initial proposal of the adaptive Metropolis shifts all 321 weights at once: a flatter likelihood and small start
    # weights, whose proposal spread is sqrt(0.09 |w|), let its chains move within 20 steps)
    sigma, scale = (1.0, 0.02) if name == 'amcmc' else (0.2, 0.3)
    C, nmcmc = 4, 20
    uq = _solver()
    inis = np.stack([scale * np.random.RandomState(20 + c).randn(uq.pdim) for c in range(C)])
    uq.fit(x, y, zflag=False, datanoise=sigma, nmcmc=nmcmc, param_ini=inis, sampler=sampler, sampler_params=params,
           seeds=range(C), engine='device', priorsigma=PS)
    assert uq.lpinfo['lparams']['priorsigma'] == PS
    r = uq.mcmc_results
    chain, lps = np.asarray(r['chain']), np.asarray(r['logpost'])
    assert chain.shape == (C, nmcmc + 1, uq.pdim) and np.isfinite(chain).all() and np.isfinite(lps).all()
    print(name, 'accrate', np.asarray(r['accrate']))
    assert not np.array_equal(chain[:, -1], chain[:, 0])
    if name != 'sghmc_mini':
        want = uq.logpost_batch(chain.reshape(-1, uq.pdim)).reshape(C, nmcmc + 1)        # the host formula with the prior
        np.testing.assert_allclose(lps, want, rtol=1e-9)
        np.testing.assert_allclose(np.asarray(r['maxpost']), uq.logpost_batch(np.asarray(r['mapparams'])), rtol=1e-9)
        # ... which is the bare likelihood plus log N(w; 0, ps^2 I)
        bare = dict(uq.lpinfo, lparams={'sigma': sigma})
        np.testing.assert_allclose(want[:, 0], uq.logpost_batch(inis, bare) + pr.log_prior(inis, PS), rtol=1e-12)
        return
    # minibatch: logpost - log prior is the minibatch estimate of the log-likelihood on the rows of the consuming step, to
    # the accuracy of the SSE: the prior is NOT rescaled by N / batch
    N, Nb, thin = 64, params['batch'], params['thin']
    op = uq._operator(uq.lpinfo)
    gs = sg.grad_scale(N, Nb, sigma)
    for k in range(nmcmc + 1):
        rows = np.stack([sg.minibatch_rows(0, k * thin, c, N, Nb) for c in range(C)])
        sse = op.sse(np.ascontiguousarray(chain[:, k]), row_idx=torch.as_tensor(rows, device="cuda")).cpu().numpy()
        want = -(gs * sse + (N / 2) * np.log(2 * np.pi) + N * np.log(sigma))
        got = lps[:, k] - pr.log_prior(chain[:, k], PS)
        assert np.all(np.abs(got - want) <= 1e-11 * gs * sse), (k, got - want)


def _begin(cur, gcur, sigma, eps, chain0, seed, step):
    L = _lib.lib()
    C, p = cur.shape
    nk = L.qn_hmc_parts(p)
    mom, q = torch.empty_like(cur), torch.empty_like(cur)
    kparts = torch.empty(C, nk, dtype=torch.float64, device=cur.device)
    st = torch.zeros(2, dtype=torch.int64, device=cur.device)
    st[0] = step
    _lib.check(L.qn_hmc_begin(cur.data_ptr(), gcur.data_ptr(), sigma, eps, C, chain0, p, seed, st.data_ptr(), mom.data_ptr(),
                              q.data_ptr(), kparts.data_ptr(), None), "qn_hmc_begin")
    torch.cuda.synchronize()
    return mom.cpu().numpy(), 0.5 * kparts.cpu().numpy().sum(axis=1)


@pytest.mark.parametrize("dims,L_", [((1, 8, 8, 1), 3), ((2, 16, 1), 1)])
def test_one_hmc_step_with_a_prior_equals_the_numpy_leapfrog_on_the_kernel_momenta(dims, L_):
    """The scheme and tolerances of the untempered one-step test of the HMC engine; the numpy target and force are the
    oracle's plus log N(w; 0, ps^2 I) and -w / ps^2."""
    x, y = _problem(N=40, d=dims[0])
    sigma, eps, seed, C, ps = 0.2, 0.003, 1234, 5, 0.6
    arch = MLPArch(dims, "tanh")
    op = BatchedMLP(arch, x, y)
    ini = 0.3 * np.random.RandomState(3).randn(C, arch.nparams)
    eng = DeviceHMC(op, sigma, epsilon=eps, L=L_, seed=seed, chain0=7, priorsigma=ps)
    r = eng.run(1, ini)
    torch.cuda.synchronize()
    cur = torch.as_tensor(ini, device="cuda")
    _, g0 = op.sse_grad(cur)
    op.prior_fold(cur, *pr.fold_constants(sigma, ps, arch.nparams), grad=g0)
    mom, kcur = _begin(cur, g0, sigma, eps, 7, eng.seed, 0)
    mod = mlp_ref.build_module(mlp_ref.MLPSpec(dims, "tanh"))
    yd = [v for v in y]
    lp = lambda w: mlp_ref.logpost(mod, w, x, yd, sigma) + pr.log_prior(w, ps)[0]
    lpg = lambda w: mlp_ref.logpostgrad(mod, w, x, yd, sigma) - w / ps ** 2
    for c in range(C):
        z = mom[c] - eps * lpg(ini[c]) / 2
        assert abs(np.sum(np.square(z)) / 2 - kcur[c]) <= 1e-12 * kcur[c]
        qq, pp = ini[c].copy(), z.copy()
        k0 = np.sum(np.square(pp)) / 2
        pp += eps * lpg(qq) / 2
        for jj in range(L_):
            qq += eps * pp
            if jj != L_ - 1:
                pp += eps * lpg(qq)
        pp += eps * lpg(qq) / 2
        k1 = np.sum(np.square(-pp)) / 2
        mh = np.exp((-lp(ini[c]) + k0) - (-lp(qq) + k1))
        np.testing.assert_allclose(r['alphas'][c, 1].item(), mh, rtol=1e-8)
        got = r['chain'][c, 1].cpu().numpy()
        if not np.array_equal(got, ini[c]):
            np.testing.assert_allclose(got, qq, rtol=1e-10, atol=1e-12)
            assert abs(r['logpost'][c, 1].item() - lp(qq)) <= 1e-10 * abs(lp(qq))
        assert abs(r['logpost'][c, 0].item() - lp(ini[c])) <= 1e-10 * abs(lp(ini[c]))
    assert (r['chain'][:, 1] != r['chain'][:, 0]).any()


def test_host_gradient_with_a_prior_equals_central_differences():
    x, y = _problem(seed=3, N=32, d=2)
    uq = _solver(hidden=(8,), d=2)
    uq.lpinfo = {'model': None, 'xd': x, 'yd': [v for v in y], 'ltype': 'classical', 'lparams': {'sigma': 0.3, 'priorsigma': 0.7}}
    p, h = uq.pdim, 1e-6
    W = 0.5 * np.random.RandomState(5).randn(3, p)
    g = uq.logpostgrad_batch(W)
    E = h * np.eye(p)
    Wp = (W[:, None, None, :] + np.stack([E, -E])[None]).reshape(-1, p)                # [3, 2, p, p] -> rows
    lp = uq.logpost_batch(Wp).reshape(3, 2, p)
    fd = (lp[:, 0] - lp[:, 1]) / (2 * h)
    # rtol as set.  The absolute floor is the rounding of the difference quotient: each log-posterior is a float64 sum over 32
    # rows of a network 8 wide, forward error <= ~64 * 2^-53 |lp| (one rounding per added term), and the two errors are divided
    # by 2 h; the truncation error, h^2 / 6 times the third derivative, is ~1e-12 and far below it
    np.testing.assert_allclose(g, fd, rtol=1e-6, atol=64 * 2.0 ** -53 * np.abs(lp).max() / h)
    bare = dict(uq.lpinfo, lparams={'sigma': 0.3})
    np.testing.assert_allclose(g, uq.logpostgrad_batch(W, bare) - W / 0.7 ** 2, rtol=1e-13, atol=1e-13)


@pytest.mark.parametrize("engine", ["hmc", "amcmc"])
def test_a_posterior_that_exists_only_because_of_the_prior(engine):
    """y = w . x + b with p = 4 weights on N = 2 rows: A^T A has rank 2, the likelihood alone is improper.  With the prior the
    posterior is N(m, S), S = (A^T A / sigma^2 + I / ps^2)^-1 (condition number 34 for this x), and has variance ps^2 along
    the two null directions of A.  Margins as in the Gaussian-posterior test of the HMC engine."""
    rs = np.random.RandomState(1)
    sigma, ps = 0.5, 1.0
    x = rs.randn(2, 3)
    A = np.hstack([x, np.ones((2, 1))])
    y = (A @ np.array([0.8, -0.5, 0.3, 0.2]) + sigma * rs.randn(2))[:, None]
    P = A.T @ A / sigma ** 2 + np.eye(4) / ps ** 2
    cov = np.linalg.inv(P)
    mean = cov @ (A.T @ y).ravel() / sigma ** 2
    assert np.linalg.matrix_rank(A.T @ A) == 2 and np.linalg.cond(cov) < 50
    arch = MLPArch((3, 1), "identity")
    assert arch.nparams == 4
    op = BatchedMLP(arch, x, y)
    C, nmcmc = 256, 400
    ini = mean + rs.randn(C, 4) @ np.linalg.cholesky(cov).T
    if engine == "hmc":
        r = DeviceHMC(op, sigma, epsilon=0.12, L=8, seed=11, priorsigma=ps).run(nmcmc, ini)
        assert 0.7 < r['accrate'].mean().item() <= 1.0
    else:
        # random-walk Metropolis with the optimally scaled proposal covariance (2.4^2 / p) S from the start
        r = DeviceAMCMC(op, sigma, cov_ini=2.4 ** 2 / 4 * cov, seed=11, priorsigma=ps).run(nmcmc, ini)
        assert 0.1 < r['accrate'].mean().item() < 0.6
    ch = r['chain'][:, 100:].cpu().numpy().reshape(-1, 4)
    se = np.sqrt(np.diag(cov) / (C * 10))                              # ~10 effective samples per chain
    got_cov = np.cov(ch.T)
    print(engine, "mean error / (5 se)", np.abs(ch.mean(axis=0) - mean) / (5 * se), "cov error", np.abs(got_cov - cov).max())
    assert np.all(np.abs(ch.mean(axis=0) - mean) < 5 * se)
    np.testing.assert_allclose(got_cov, cov, rtol=0.15, atol=0.1 * np.abs(cov).max())
    V = np.linalg.svd(A)[2][2:].T                                      # [4, 2]: the null directions of A
    assert np.allclose(A @ V, 0.0, atol=1e-12)
    np.testing.assert_allclose(V.T @ got_cov @ V, ps ** 2 * np.eye(2), rtol=0.15, atol=0.1 * np.abs(cov).max())
    # the stored trace is the Gaussian's log-density up to the evidence: constant offset over all states
    off = r['logpost'][:, 100:].cpu().numpy().ravel() + 0.5 * np.einsum('ni,ij,nj->n', ch - mean, P, ch - mean)
    assert np.ptp(off) < 1e-8


def _engines(op, sigma, **kw):
    return {'amcmc': lambda: DeviceAMCMC(op, sigma, gamma=0.1, seed=3, **kw),
            'hmc': lambda: DeviceHMC(op, sigma, epsilon=0.002, L=2, seed=3, **kw),
            'mala': lambda: DeviceMALA(op, sigma, epsilon=0.003, seed=3, **kw),
            'sghmc': lambda: DeviceSGHMC(op, sigma, eta=2e-6, alpha=0.1, batch=16, seed=3, **kw),
            'sgld': lambda: DeviceSGLD(op, sigma, eta=2e-6, batch=16, seed=3, **kw)}


@pytest.mark.parametrize("name", ['amcmc', 'hmc', 'mala', 'sghmc', 'sgld'])
def test_priorsigma_none_is_the_engine_without_the_argument_bit_for_bit(name):
    x, y = _problem(N=64)
    arch = MLPArch((1, 16, 16, 1), "tanh")
    op = BatchedMLP(arch, x, y)
    ini = np.stack([np.random.RandomState(70 + c).rand(arch.nparams) for c in range(4)])
    a = _engines(op, 0.2)[name]().run(6, ini)
    b = _engines(op, 0.2, priorsigma=None)[name]().run(6, ini)
    c = _engines(op, 0.2, priorsigma=PS)[name]().run(6, ini)
    for k in KEYS:
        assert torch.equal(a[k], b[k]), k
    assert not torch.equal(a['logpost'], c['logpost'])                    # (and a prior is not a no-op)


def test_graph_replay_with_a_prior_equals_direct_launches_bit_for_bit():
    x, y = _problem(N=64)
    arch = MLPArch((1, 16, 16, 1), "tanh")
    op = BatchedMLP(arch, x, y)
    ini = np.stack([np.random.RandomState(70 + c).rand(arch.nparams) for c in range(4)])
    d = DeviceHMC(op, 0.2, epsilon=0.002, L=2, seed=5, priorsigma=PS).run(6, ini)
    g = DeviceHMC(op, 0.2, epsilon=0.002, L=2, seed=5, priorsigma=PS, use_graph=True).run(6, ini)
    for k in d:
        assert torch.equal(d[k], g[k]), k


def test_chain_groups_with_a_prior_on_the_fused_kernels_are_bit_identical():
    rs = np.random.RandomState(3)
    N, C = 2048, 64
    x = rs.rand(N, 1) * 2 - 1
    y = np.sin(3 * x) + 0.1 * rs.randn(N, 1)
    arch = MLPArch((1, 64, 64, 64, 1), "tanh")
    op = BatchedMLP(arch, x, y)
    assert op.arith(C) == _lib.ARITH_I8_FUSED
    ini = np.stack([np.random.RandomState(900 + c).rand(arch.nparams) for c in range(C)])
    kw = dict(gamma=0.05, t0=30, tadapt=60, seed=21, priorsigma=PS)
    one = DeviceAMCMC(op, 0.1, groups=1, **kw).run(100, ini)
    two = DeviceAMCMC(op, 0.1, groups=2, **kw).run(100, ini)
    for k in KEYS:
        assert torch.equal(one[k], two[k]), k
    assert (one['accrate'] > 0).all() and (one['accrate'] < 1).all()


@pytest.mark.parametrize("engine", ["device", "host"])
def test_through_the_solver(engine):
    x, y = _problem(seed=2, N=64)
    uq = _solver(hidden=(6,))
    inis = np.stack([0.1 * np.random.RandomState(30 + c).randn(uq.pdim) for c in range(8)])
    uq.fit(x, y, zflag=False, datanoise=0.3, nmcmc=30, param_ini=inis, sampler='hmc', sampler_params={'epsilon': 0.01, 'L': 3},
           seeds=range(8), engine=engine, priorsigma=0.5, diagnostics=True)
    assert uq.lpinfo['lparams']['priorsigma'] == 0.5
    assert uq.samples.shape == (8, 31, uq.pdim) and np.isfinite(uq.samples).all()
    assert np.shape(uq.diagnostics['params']['rhat']) == (uq.pdim,)
    np.testing.assert_allclose(np.asarray(uq.mcmc_results['maxpost']), uq.logpost_batch(np.asarray(uq.cmode)), rtol=1e-9)
    assert 0.0 < np.mean(uq.mcmc_results['accrate']) <= 1.0
