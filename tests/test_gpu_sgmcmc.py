"""GPU: the stochastic-gradient samplers (qn_sg_rows / qn_sg_step around the batched gradient kernel; `DeviceSGLD`,
`DeviceSGHMC`).  The rows are checked bit for bit against the numpy restatement, the update against `sgmcmc.sg_step` fed the
kernel's own gradient, the noise in distribution and for its keys, the chains for independence from the way they are split,
graph replay, thinning and the cyclic schedule, and the samplers in distribution on a Gaussian posterior."""
import numpy as np
import pytest
import torch

from quinn_amd import _lib
from quinn_amd.mcmc import sgmcmc as sg
from quinn_amd.mcmc.device_sgmcmc import DeviceSGHMC, DeviceSGLD
from quinn_amd.ops import BatchedMLP, MLPArch

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


def _problem(seed=0, N=48, d=1):
    rs = np.random.RandomState(seed)
    x = rs.rand(N, d) * 6 - 3
    y = np.sin(x).sum(axis=1, keepdims=True) + 0.1 * rs.randn(N, 1)
    return x, y


def _rows(C, Nb, N, chain0, seed, step, counter=0):
    """qn_sg_rows through the C ABI: int32 device tensor [C, Nb] of inner step `step` = device counter + host offset."""
    rows = torch.full((C, Nb), -1, dtype=torch.int32, device="cuda")
    st = torch.tensor([counter, -7], dtype=torch.int64, device="cuda")
    _lib.check(_lib.lib().qn_sg_rows(rows.data_ptr(), C, Nb, N, chain0, seed, st.data_ptr(), step - counter, None), "qn_sg_rows")
    torch.cuda.synchronize()
    return rows


def _step(theta, v, g, sse, *, sigma, N, Nb, eta, alpha, T=1.0, schedule=0, K=0, ef=0.0, thin=1, final=0, chain0=0, nstore=4,
          seed=1, t=0, par=0, rows=None, chain=None, thop=None):
    """qn_sg_step through the C ABI on copies of theta / v: dict of what it wrote."""
    C, p = theta.shape
    dev = theta.device
    th = theta.clone()
    vv = None if v is None else v.clone()
    best = torch.zeros_like(th)
    best_lp = torch.full((2, C), -np.inf, dtype=torch.float64, device=dev)
    lps = torch.full((C, nstore + 1), np.nan, dtype=torch.float64, device=dev)
    st = torch.full((2,), -99, dtype=torch.int64, device=dev)
    st[par] = t
    ptr = lambda a: None if a is None else a.data_ptr()
    qdt = _lib.QN_F32 if g.dtype == torch.float32 else _lib.QN_F64
    _lib.check(_lib.lib().qn_sg_step(th.data_ptr(), ptr(vv), g.data_ptr(), qdt, sse.data_ptr(), sigma, N, Nb, eta, alpha, T, schedule,
                                     K, ef, thin, final, C, chain0, p, nstore, seed, ptr(thop), best.data_ptr(), best_lp.data_ptr(),
                                     ptr(chain), lps.data_ptr(), ptr(rows), st.data_ptr(), par, None), "qn_sg_step")
    torch.cuda.synchronize()
    return {'theta': th, 'v': vv, 'best': best, 'best_lp': best_lp, 'lps': lps, 'step': st}


def test_rows_equal_the_numpy_restatement_bit_for_bit():
    C, chain0, seed = 3, 5, 77
    for N in (1, 7, 4096, 100003):
        for Nb in (1, 3, 4, 5, 257):
            for step, counter in ((0, 0), (1, 1), (12345, 12000), (12345, 0)):
                got = _rows(C, Nb, N, chain0, seed, step, counter).cpu().numpy()
                want = np.stack([sg.minibatch_rows(seed, step, chain0 + c, N, Nb) for c in range(C)])
                assert np.array_equal(got, want), (N, Nb, step, counter)


def test_the_step_kernel_writes_the_next_steps_rows():
    C, p, N, chain0, seed = 3, 13, 100003, 5, 9
    theta = torch.zeros(C, p, dtype=torch.float64, device="cuda")
    g, sse = torch.zeros_like(theta), torch.zeros(C, dtype=torch.float64, device="cuda")
    for Nb in (1, 5, 8, 257):
        for t in (0, 7, 12344):
            par = t & 1
            rows = torch.full((2, C, Nb), -1, dtype=torch.int32, device="cuda")
            r = _step(theta, None, g, sse, sigma=0.5, N=N, Nb=Nb, eta=1e-3, alpha=1.0, chain0=chain0, seed=seed, t=t, par=par,
                      rows=rows)
            assert torch.equal(rows[1 - par], _rows(C, Nb, N, chain0, seed, t + 1)), (Nb, t)
            assert torch.all(rows[par] == -1)                              # the half the gradient call of step t read
            assert r['step'][1 - par].item() == t + 1 and r['step'][par].item() == t
            # a final call draws nothing and leaves the counter where it is
            rows.fill_(-1)
            r = _step(theta, None, g, sse, sigma=0.5, N=N, Nb=Nb, eta=1e-3, alpha=1.0, chain0=chain0, seed=seed, t=t, par=par,
                      rows=rows, final=1)
            assert torch.all(rows == -1) and r['step'][1 - par].item() == t and torch.equal(r['theta'], theta)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("dims", [(1, 5, 1), (2, 3, 1), (1, 32, 32, 1)])
def test_one_step_without_noise_equals_the_numpy_update_on_the_kernels_gradient(dims, dtype):
    """p = 16 (even), 13 (odd: the lone last element) and 1153 (odd, several workgroups per chain).  temperature = 0; the
    update is three multiply-adds whose contraction is the compiler's choice: bound 8 * 2^-53 times the element's largest term
    (|theta|, |(1 - alpha) v|, |eta g|)."""
    N, sigma, eta, seed, chain0 = 23, 0.5, 1e-3, 31, 2
    x, y = _problem(N=N, d=dims[0])
    arch = MLPArch(dims, "tanh")
    p = arch.nparams
    assert p == {(1, 5, 1): 16, (2, 3, 1): 13, (1, 32, 32, 1): 1153}[dims]
    op = BatchedMLP(arch, x, y, dtype=dtype)
    rs = np.random.RandomState(3)
    for C in (1, 3):
        th0, v0 = 0.3 * rs.randn(C, p), 0.01 * rs.randn(C, p)
        theta, v = torch.as_tensor(th0, device="cuda"), torch.as_tensor(v0, device="cuda")
        for batch in (None, 5):
            Nb = N if batch is None else batch
            rows = None if batch is None else _rows(C, Nb, N, chain0, seed, 0)
            sse, g = op.sse_grad(theta.to(op.tdt), row_idx=rows)
            gh, gs = g.double().cpu().numpy(), sg.grad_scale(N, Nb, sigma)
            for alpha in (1.0, 0.1):
                thop = torch.zeros(C, p, dtype=torch.float32, device="cuda") if dtype == "float32" else None
                r = _step(theta, v, g, sse, sigma=sigma, N=N, Nb=Nb, eta=eta, alpha=alpha, T=0.0, chain0=chain0, seed=seed,
                          thop=thop)
                t1, v1 = sg.sg_step(th0, v0, gh, 0.0, eta, alpha, gs, 0.0)
                big_v = np.maximum(np.abs((1 - alpha) * v0), np.abs(eta * gs * gh))
                big = np.maximum(np.abs(th0), big_v)
                assert np.all(np.abs(r['theta'].cpu().numpy() - t1) <= 8 * U * big), (C, batch, alpha)
                if alpha == 1.0:
                    assert torch.equal(r['v'], v)                           # SGLD never touches v
                else:
                    assert np.all(np.abs(r['v'].cpu().numpy() - v1) <= 8 * U * big_v), (C, batch, alpha)
                if thop is not None:                                        # what a float32 operator's next call reads
                    assert torch.equal(thop, r['theta'].float())
                # the log-posterior trace of the incoming state is the minibatch estimate, and the first state is the best
                lp = -(gs * sse.cpu().numpy() + (N / 2) * np.log(2 * np.pi) + N * np.log(sigma))
                np.testing.assert_allclose(r['lps'][:, 0].cpu().numpy(), lp, rtol=1e-15)
                assert torch.equal(r['best'], theta) and torch.equal(r['best_lp'][1], r['lps'][:, 0])
        # the engine runs the same two launches: its first step from v = 0, its second from the v of the first
        for alpha, batch in ((0.1, 5), (1.0, None)):
            Nb = N if batch is None else batch
            gs = sg.grad_scale(N, Nb, sigma)
            res = DeviceSGHMC(op, sigma, eta=eta, alpha=alpha, batch=batch, temperature=0.0, seed=seed, chain0=chain0).run(2, th0)
            ch = res['chain'].cpu().numpy()
            vn = np.zeros_like(th0)
            for t in range(2):
                cur = res['chain'][:, t].contiguous()
                rows = None if batch is None else _rows(C, Nb, N, chain0, seed, t)
                _, g = op.sse_grad(cur.to(op.tdt), row_idx=rows)
                gh = g.double().cpu().numpy()
                big = np.maximum(np.abs(ch[:, t]), np.maximum(np.abs((1 - alpha) * vn), np.abs(eta * gs * gh)))
                want, vn = sg.sg_step(ch[:, t], vn, gh, 0.0, eta, alpha, gs, 0.0)
                assert np.all(np.abs(ch[:, t + 1] - want) <= 8 * U * big), (alpha, batch, t)
            assert torch.all(res['accrate'] == 1) and torch.all(res['alphas'] == 1)


def test_noise_is_standard_normal_and_keyed_by_seed_step_and_global_chain():
    C, p, eta, seed, t = 64, 1153, 0.02, 42, 5
    rs = np.random.RandomState(0)
    theta = torch.as_tensor(rs.randn(C, p), device="cuda")
    g = torch.as_tensor(rs.randn(C, p), device="cuda")
    sse = torch.zeros(C, dtype=torch.float64, device="cuda")
    sigma = np.sqrt(0.5)                                                    # N = Nb: g enters with the factor 1
    kw = dict(sigma=sigma, N=10, Nb=10, eta=eta, alpha=1.0, T=1.0, par=1)
    new = lambda th, gg, **k: _step(th, None, gg, sse[:th.shape[0]], **{**kw, **k})['theta']
    a = new(theta, g, seed=seed, t=t, chain0=0)
    gs = sg.grad_scale(10, 10, sigma)
    z = ((a - theta + eta * gs * g) / np.sqrt(2 * eta)).cpu().numpy().ravel()
    n = z.size
    assert abs(z.mean()) < 5 / np.sqrt(n) and abs(z.var() - 1) < 5 * np.sqrt(2 / n) and abs((z ** 4).mean() - 3) < 5 * np.sqrt(96 / n)
    assert torch.equal(a, new(theta, g, seed=seed, t=t, chain0=0))
    # chains 10..19 of a launch that starts at chain 10 == chains 10..19 of the launch that starts at 0
    assert torch.equal(new(theta[10:20].contiguous(), g[10:20].contiguous(), seed=seed, t=t, chain0=10), a[10:20])
    for other in (dict(seed=seed + 1, t=t, chain0=0), dict(seed=seed, t=t + 1, chain0=0), dict(seed=seed, t=t, chain0=1)):
        b = new(theta, g, **other)
        assert not torch.any(b == a), other                                 # every element's draw changes
    # temperature 0: no noise at all
    assert torch.equal(new(theta, g, seed=seed, t=t, chain0=0, T=0.0), new(theta, g, seed=seed + 1, t=t + 1, chain0=3, T=0.0))


KEYS = ('chain', 'logpost', 'alphas', 'accrate', 'mapparams', 'maxpost')


def _small(batch=16, C=6):
    x, y = _problem(N=64)
    arch = MLPArch((1, 16, 16, 1), "tanh")
    ini = np.stack([np.random.RandomState(50 + c).rand(arch.nparams) for c in range(C)])
    return arch, x, y, ini


def test_chains_do_not_depend_on_how_they_are_split():
    arch, x, y, ini = _small()
    kw = dict(eta=2e-5, alpha=0.1, batch=16, seed=9)
    whole = DeviceSGHMC(BatchedMLP(arch, x, y), 0.2, chain0=0, **kw).run(12, ini)
    parts = []
    for c0 in (0, 3):
        op = BatchedMLP(arch, x, y)
        op.set_plan_batch(6)                    # split every chain's rows as the launch of all six chains does
        parts.append(DeviceSGHMC(op, 0.2, chain0=c0, **kw).run(12, ini[c0:c0 + 3]))
    for k in KEYS:
        assert torch.equal(torch.cat([parts[0][k], parts[1][k]]), whole[k]), k
    two = DeviceSGHMC(BatchedMLP(arch, x, y), 0.2, chain0=0, groups=2, **kw).run(12, ini)
    for k in KEYS:
        assert torch.equal(two[k], whole[k]), k
    assert torch.isfinite(whole['chain']).all() and not torch.equal(whole['chain'][:, 1], whole['chain'][:, 0])


def test_graph_replay_equals_direct_launches_bit_for_bit():
    arch, x, y, ini = _small(C=4)
    op = BatchedMLP(arch, x, y)
    for thin in (2, 1):                 # 18 inner steps: all replayed; 9: an un-captured last step; both end with the final call
        kw = dict(eta=2e-5, alpha=0.1, batch=16, thin=thin, schedule='cyclic', cycles=2, explore_frac=0.25, seed=5)
        d = DeviceSGHMC(op, 0.2, **kw).run(9, ini[:4])
        g = DeviceSGHMC(op, 0.2, use_graph=True, **kw).run(9, ini[:4])
        for k in KEYS:
            assert torch.equal(d[k], g[k]), (thin, k)
        assert torch.isfinite(d['logpost']).all()


def test_thinning_stores_every_thin_th_state_and_its_minibatch_log_posterior():
    arch, x, y, ini = _small(C=3)
    N, Nb, sigma, seed, chain0 = 64, 16, 0.2, 4, 2
    op = BatchedMLP(arch, x, y)
    kw = dict(eta=2e-5, alpha=0.1, batch=Nb, seed=seed, chain0=chain0)
    full = DeviceSGHMC(op, sigma, thin=1, **kw).run(12, ini[:3])
    thin = DeviceSGHMC(op, sigma, thin=3, **kw).run(4, ini[:3])
    assert thin['chain'].shape == (3, 5, arch.nparams) and thin['logpost'].shape == (3, 5)
    assert torch.equal(thin['chain'], full['chain'][:, ::3]) and torch.equal(thin['logpost'], full['logpost'][:, ::3])
    # the last row's log-posterior: the minibatch estimate on the rows of inner step 12 (the accuracy of the SSE, 1e-11)
    rows = _rows(3, Nb, N, chain0, seed, 12)
    sse = op.sse(thin['chain'][:, -1].contiguous(), row_idx=rows).cpu().numpy()
    gs = sg.grad_scale(N, Nb, sigma)
    want = -(gs * sse + (N / 2) * np.log(2 * np.pi) + N * np.log(sigma))
    for r in (thin, full):
        assert np.all(np.abs(r['logpost'][:, -1].cpu().numpy() - want) <= 1e-11 * gs * sse)
    # MAP bookkeeping: the best stored state by that estimate
    lp = full['logpost'].cpu().numpy()
    assert np.array_equal(full['maxpost'].cpu().numpy(), lp.max(axis=1))
    for c in range(3):
        assert torch.equal(full['mapparams'][c], full['chain'][c, int(lp[c].argmax())])


def test_cyclic_schedule_follows_the_device_step_counter():
    """Two cycles of 4 inner steps, explore_frac = 0.5.  Without noise the chain is the numpy recursion with `step_size(t)` on
    the kernel's own gradients; the device cosine and numpy's may differ by an ulp or two and v carries its rounding along
    (geometric sum 1 / alpha = 2), so the bound is 64 * 2^-53 of the element's largest term -- a wrong step size or a wrong
    cycle position shows at 1e-2.  With noise, steps 0, 1 of each cycle stay deterministic and steps 2, 3 do not."""
    arch, x, y, ini = _small(C=3)
    N, Nb, sigma, seed, K, eta0 = 64, 8, 0.2, 13, 4, 4e-5
    op = BatchedMLP(arch, x, y)
    gs = sg.grad_scale(N, Nb, sigma)
    assert sg.step_size(1, eta0, 'cyclic', K) < 0.9 * eta0

    def grad(state, t):
        rows = torch.as_tensor(np.stack([sg.minibatch_rows(seed, t, c, N, Nb) for c in range(3)]), device="cuda")
        return op.sse_grad(state.contiguous(), row_idx=rows)[1].cpu().numpy()

    kw = dict(batch=Nb, schedule='cyclic', cycles=2, explore_frac=0.5, seed=seed)
    alpha = 0.5
    r0 = DeviceSGHMC(op, sigma, eta=eta0, alpha=alpha, temperature=0.0, **kw).run(8, ini[:3])
    ch = r0['chain'].cpu().numpy()
    v = np.zeros_like(ch[:, 0])
    for t in range(8):
        g, eta = grad(r0['chain'][:, t], t), sg.step_size(t, eta0, 'cyclic', K)
        big = np.maximum(np.abs(ch[:, t]), np.maximum(np.abs(v), np.abs(eta * gs * g)))
        want, v = sg.sg_step(ch[:, t], v, g, 0.0, eta, alpha, gs, 0.0)
        assert np.all(np.abs(ch[:, t + 1] - want) <= 64 * U * big), t
    # SGLD with noise: a step is deterministic exactly where the mask is off
    r1 = DeviceSGLD(op, sigma, eta=eta0, temperature=1.0, **kw).run(8, ini[:3])
    ch = r1['chain'].cpu().numpy()
    for t in range(8):
        g, eta = grad(r1['chain'][:, t], t), sg.step_size(t, eta0, 'cyclic', K)
        want, _ = sg.sg_step(ch[:, t], None, g, 0.0, eta, 1.0, gs, 0.0)
        big = np.maximum(np.abs(ch[:, t]), np.abs(eta * gs * g))
        same = np.abs(ch[:, t + 1] - want) <= 64 * U * big
        if sg.noise_on(t, K, 0.5):
            assert t % K in (2, 3) and not same.any(), t
            assert np.all(np.abs(ch[:, t + 1] - want) < 8 * np.sqrt(2 * eta))      # ... by a draw of sqrt(2 eta) z
        else:
            assert t % K in (0, 1) and same.all(), t
    r1c = DeviceSGLD(op, sigma, eta=eta0, temperature=0.0, **kw).run(8, ini[:3])
    assert torch.equal(r1c['chain'][:, :3], r1['chain'][:, :3]) and not torch.equal(r1c['chain'][:, 3], r1['chain'][:, 3])


# ---- Gaussian target -------------------------------------------------------------------------------------------------------
G_N, G_SIGMA, G_C, G_NMCMC, G_BURN = 50, 0.5, 256, 2000, 200


def _linear_model():
    """The linear model of test_gpu_device_hmc.test_gaussian_posterior_moments: y = w x + b, Gaussian posterior over (w, b)."""
    rs = np.random.RandomState(1)
    x = rs.randn(G_N, 1)
    y = 1.5 * x - 0.7 + G_SIGMA * rs.randn(G_N, 1)
    A = np.hstack([x, np.ones((G_N, 1))])
    Lam = A.T @ A / G_SIGMA ** 2
    mean = np.linalg.solve(A.T @ A, A.T @ y).ravel()
    eta = 0.1 / np.linalg.eigvalsh(Lam).max()
    return x, y, A, Lam, mean, eta, mean + 0.1 * rs.randn(G_C, 2)


def _deviations(chain, mean, want_cov):
    """(mean deviation in posterior standard deviations, covariance deviation relative to sqrt(C_ii C_jj)), pooled over the
    chains after the burn-in."""
    s = chain[:, G_BURN:].reshape(-1, 2)
    sd = np.sqrt(np.diag(want_cov))
    return np.max(np.abs(s.mean(axis=0) - mean) / sd), np.max(np.abs(np.cov(s.T) - want_cov) / np.outer(sd, sd))


def cpu_deviations(seed, batch=None):
    """The numpy recursion of `sgmcmc.sg_step` with the test's chain count and length (not run by the tests: it is where the
    bounds below come from).  batch: rows per step, drawn with replacement by numpy."""
    x, y, A, Lam, mean, eta, ini = _linear_model()
    rs = np.random.RandomState(1000 + seed)
    th = ini.copy()
    chain = np.empty((G_C, G_NMCMC + 1, 2))
    chain[:, 0] = th
    Nb = G_N if batch is None else batch
    gs = sg.grad_scale(G_N, Nb, G_SIGMA)
    for t in range(G_NMCMC):
        if batch is None:
            grad = 2 * (th @ A.T - y.ravel()) @ A                           # d SSE / d theta
        else:
            idx = rs.randint(0, G_N, size=(G_C, Nb))
            Ab = A[idx]                                                     # [C, Nb, 2]
            grad = 2 * np.einsum('cn,cnk->ck', np.einsum('cnk,ck->cn', Ab, th) - y.ravel()[idx], Ab)
        th, _ = sg.sg_step(th, None, grad, rs.randn(G_C, 2), eta, 1.0, gs)
        chain[:, t + 1] = th
    return _deviations(chain, mean, sg.ula_cov(Lam, eta))


# largest deviations of `cpu_deviations` over seeds 0..19 (mean / covariance, full batch; mean, batch = N // 8 = 6), and the
# bounds: 4 x those.  (With batch = 6 the same runs' covariance deviates by up to 0.284: minibatch noise, not pinned.)
CPU_MEAN_FULL, CPU_COV_FULL, CPU_MEAN_MINI = 0.0119774, 0.0138966, 0.0138967


def test_gaussian_target_full_batch_has_the_least_squares_mean_and_the_ula_covariance():
    """Full-batch SGLD, 256 chains x 2000 steps (200 discarded), eta lambda_max = 0.1: pooled mean = least-squares solution,
    pooled covariance = `ula_cov(Lambda, eta)` -- the closed form for this eta, not the exact posterior.  Tolerance: the numpy
    recursion (`cpu_deviations`, same chain count and length) over 20 seeds deviates by at most CPU_MEAN_FULL = 0.01198
    posterior standard deviations in the mean and CPU_COV_FULL = 0.01390 (relative to sqrt(C_ii C_jj)) in the covariance; the
    bounds are 4 x those Monte-Carlo figures: 0.04791 and 0.05559."""
    x, y, A, Lam, mean, eta, ini = _linear_model()
    op = BatchedMLP(MLPArch((1, 1), "identity"), x, y)
    r = DeviceSGLD(op, G_SIGMA, eta=eta, seed=11).run(G_NMCMC, ini)
    dm, dc = _deviations(r['chain'].cpu().numpy(), mean, sg.ula_cov(Lam, eta))
    print("gaussian target, full batch: mean deviation %.4g (bound %.4g), covariance deviation %.4g (bound %.4g)"
          % (dm, 4 * CPU_MEAN_FULL, dc, 4 * CPU_COV_FULL))
    assert dm <= 4 * CPU_MEAN_FULL and dc <= 4 * CPU_COV_FULL
    # full batch: the trace is the exact log-posterior, and the MAP estimate is its maximum
    lp = r['logpost'].cpu().numpy()
    sse = op.sse(r['chain'][:, -1].contiguous()).cpu().numpy()
    np.testing.assert_allclose(lp[:, -1], -(0.5 * sse / G_SIGMA ** 2 + (G_N / 2) * np.log(2 * np.pi) + G_N * np.log(G_SIGMA)),
                               rtol=1e-11)
    assert np.array_equal(r['maxpost'].cpu().numpy(), lp.max(axis=1))


def test_gaussian_target_minibatch_has_the_least_squares_mean():
    """batch = N // 8 = 6 rows of 50 (50 / 8 is no integer): only the mean is pinned -- the minibatch gradient is unbiased and
    linear in theta, so the stationary mean is the least-squares solution, while its noise inflates the covariance.  Bound: 4 x
    CPU_MEAN_MINI = 4 x 0.01390 = 0.05559, the largest deviation (in standard deviations of `ula_cov`) of
    `cpu_deviations(seed, batch=6)` over 20 seeds."""
    x, y, A, Lam, mean, eta, ini = _linear_model()
    op = BatchedMLP(MLPArch((1, 1), "identity"), x, y)
    r = DeviceSGLD(op, G_SIGMA, eta=eta, batch=G_N // 8, seed=12).run(G_NMCMC, ini)
    ch = r['chain'].cpu().numpy()
    dm, dc = _deviations(ch, mean, sg.ula_cov(Lam, eta))
    print("gaussian target, batch 6: mean deviation %.4g (bound %.4g); covariance deviation %.4g (not pinned)"
          % (dm, 4 * CPU_MEAN_MINI, dc))
    assert np.isfinite(ch).all() and dm <= 4 * CPU_MEAN_MINI


@pytest.mark.parametrize("sampler", ["sghmc", "sgld"])
def test_through_the_solver(sampler):
    from quinn_amd.nns.mlp import MLP
    from quinn_amd.solvers.nn_mcmc import NN_MCMC
    x, y = _problem(seed=2, N=64)
    torch.manual_seed(0)
    s = NN_MCMC(MLP(1, 1, (16, 16), activ="tanh"), verbose=False)
    params = {'eta': 2e-6, 'batch': 32, 'thin': 2}
    if sampler == 'sghmc':
        params['alpha'] = 0.1
    inis = np.stack([0.3 * np.random.RandomState(20 + c).randn(s.pdim) for c in range(4)])
    s.fit(x, y, zflag=False, datanoise=0.3, nmcmc=20, param_ini=inis, sampler=sampler, sampler_params=params, seeds=range(4),
          engine='device', diagnostics=True)
    r = s.mcmc_results
    assert s.samples.shape == (4, 21, s.pdim) and r['logpost'].shape == (4, 21) and r['alphas'].shape == (4, 21)
    for k in ('chain', 'logpost', 'mapparams', 'maxpost'):
        assert np.isfinite(np.asarray(r[k])).all(), k
    assert np.all(r['accrate'] == 1) and np.all(r['alphas'] == 1)
    assert np.array_equal(s.samples[:, 0], inis) and not np.array_equal(s.samples[:, 1], inis)
    assert np.shape(s.diagnostics['params']['rhat']) == (s.pdim,) and np.shape(s.diagnostics['logpost']['rhat']) == (1,)
    ens = s.predict_ens(x, nens=4, nburn=4, chain='all')
    assert ens.shape == (4, 64, 1) and np.isfinite(ens).all()
    m, var, _ = s.predict_mom_sample(x, msc=1, nsam=4, nburn=4, chain='all')
    assert m.shape == (64, 1) and np.isfinite(m).all() and np.all(var >= 0)
