"""GPU: device HMC / MALA warm-up (csrc/qn_hmc_leap.hip, csrc/qn_hmc_adapt.hip).  qn_hmc_begin_s / qn_hmc_leap_s against the fixed-step kernels bit
for bit (scale NULL / 1, equal step sizes) and against the numpy whitened leapfrog (different step sizes, random scale);
qn_hmc_adapt against the numpy recurrences of quinn_amd/mcmc/adapt.py; the engine on a Gaussian posterior from a step size
at which the unadapted engine accepts nothing; independence from the chain split, graph replay, and the solver."""
import numpy as np
import pytest
import torch

from quinn_amd import _lib
from quinn_amd.mcmc.device_hmc import DeviceHMC
from quinn_amd.mcmc.device_mala import DeviceMALA
from quinn_amd.ops import BatchedMLP, MLPArch

pytestmark = pytest.mark.gpu
F64 = torch.float64


def _problem(seed=0, N=48, d=1):
    rs = np.random.RandomState(seed)
    x = rs.rand(N, d) * 6 - 3
    y = np.sin(x).sum(axis=1, keepdims=True) + 0.1 * rs.randn(N, 1)
    return x, y


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=F64, device="cuda")


def _ptr(t):
    return None if t is None else t.data_ptr()


def _one_step(kind, cur, gcur, grads, sigma, eps, scale, chain0, seed, step, f32=False, beta=None):
    """One leapfrog trajectory through the C ABI with the given gradient arrays (one per leapfrog step) -> mom, q, K_cur
    partials, K_prop partials (host).  kind 'fixed': qn_hmc_begin / qn_hmc_leap with the scalar eps; 's': the _s calls with
    eps [C] and scale [C, p] or None on the device; 't': the _t calls with those and beta [C] or None."""
    L = _lib.lib()
    C, p = cur.shape
    nk = L.qn_hmc_parts(p)
    mom, q = torch.empty_like(cur), torch.empty_like(cur)
    kc, kp = torch.zeros(C, nk, dtype=F64, device="cuda"), torch.zeros(C, nk, dtype=F64, device="cuda")
    st = torch.zeros(2, dtype=torch.int64, device="cuda")
    st[0] = step
    if kind == 'fixed':
        _lib.check(L.qn_hmc_begin(cur.data_ptr(), gcur.data_ptr(), sigma, eps, C, chain0, p, seed, st.data_ptr(),
                                  mom.data_ptr(), q.data_ptr(), kc.data_ptr(), None), "qn_hmc_begin")
    elif kind == 't':
        _lib.check(L.qn_hmc_begin_t(cur.data_ptr(), gcur.data_ptr(), sigma, eps.data_ptr(), _ptr(scale), _ptr(beta), C, chain0,
                                    p, seed, st.data_ptr(), mom.data_ptr(), q.data_ptr(), kc.data_ptr(), None), "qn_hmc_begin_t")
    else:
        _lib.check(L.qn_hmc_begin_s(cur.data_ptr(), gcur.data_ptr(), sigma, eps.data_ptr(), _ptr(scale), C, chain0, p, seed,
                                    st.data_ptr(), mom.data_ptr(), q.data_ptr(), kc.data_ptr(), None), "qn_hmc_begin_s")
    for j, g in enumerate(grads):
        last = int(j == len(grads) - 1)
        g = g.float() if f32 else g
        dt = _lib.QN_F32 if f32 else _lib.QN_F64
        if kind == 'fixed':
            _lib.check(L.qn_hmc_leap(g.data_ptr(), dt, sigma, eps, last, C, p, mom.data_ptr(), q.data_ptr(), kp.data_ptr(),
                                     None), "qn_hmc_leap")
        elif kind == 't':
            _lib.check(L.qn_hmc_leap_t(g.data_ptr(), dt, sigma, eps.data_ptr(), _ptr(scale), _ptr(beta), last, C, p,
                                       mom.data_ptr(), q.data_ptr(), kp.data_ptr(), None), "qn_hmc_leap_t")
        else:
            _lib.check(L.qn_hmc_leap_s(g.data_ptr(), dt, sigma, eps.data_ptr(), _ptr(scale), last, C, p, mom.data_ptr(),
                                       q.data_ptr(), kp.data_ptr(), None), "qn_hmc_leap_s")
    torch.cuda.synchronize()
    return mom.cpu().numpy(), q.cpu().numpy(), kc.cpu().numpy(), kp.cpu().numpy()


@pytest.mark.parametrize("dims", [(1, 8, 8, 1), (2, 16, 1), (1, 64, 64, 1)])
@pytest.mark.parametrize("L_", [1, 3])
def test_scaled_kernels_equal_the_fixed_step_kernels_bit_for_bit(dims, L_):
    """p = 97 (odd, one workgroup per chain), 65, 4353 (five workgroups per chain): scale NULL and scale = 1 with equal step
    sizes give qn_hmc_begin / qn_hmc_leap's momenta, positions and both kinetic partial sums, float64 and float32 gradients."""
    p = MLPArch(dims, "tanh").nparams
    assert p == {(1, 8, 8, 1): 97, (2, 16, 1): 65, (1, 64, 64, 1): 4353}[dims]
    assert _lib.lib().qn_hmc_parts(p) == (5 if p == 4353 else 1)
    rs = np.random.RandomState(p + L_)
    C, sigma, eps, seed = 3, 0.2, 0.0123, 991
    cur, gcur = _dev(0.3 * rs.randn(C, p)), _dev(5 * rs.randn(C, p))
    grads = [_dev(5 * rs.randn(C, p)) for _ in range(L_)]
    epsv = torch.full((C,), eps, dtype=F64, device="cuda")
    for f32 in (False, True):
        ref = _one_step('fixed', cur, gcur, grads, sigma, eps, None, 4, seed, 6, f32)
        for scale in (None, torch.ones(C, p, dtype=F64, device="cuda")):
            got = _one_step('s', cur, gcur, grads, sigma, epsv, scale, 4, seed, 6, f32)
            for name, a, b in zip(("mom", "q", "kin_cur", "kin_prop"), got, ref):
                assert np.array_equal(a, b), (name, f32, scale is None)
    assert np.all(ref[2] > 0) and np.all(ref[3] > 0)


@pytest.mark.parametrize("dims", [(1, 8, 8, 1), (1, 64, 64, 1)])
@pytest.mark.parametrize("L_", [1, 3])
def test_tempered_kernels_without_a_temperature_equal_both_others_bit_for_bit(dims, L_):
    """p = 97 (odd tail, one workgroup per chain) and 4353 (five workgroups), C = 3: qn_hmc_begin_t / qn_hmc_leap_t with beta
    NULL and beta = 1, each with scale NULL and scale = 1, give the momenta, positions and both kinetic partial sums of the
    fixed-step and of the _s calls, float64 and float32 gradients: all three are one kernel."""
    p = MLPArch(dims, "tanh").nparams
    assert p == {(1, 8, 8, 1): 97, (1, 64, 64, 1): 4353}[dims]
    assert _lib.lib().qn_hmc_parts(p) == (5 if p == 4353 else 1)
    rs = np.random.RandomState(p + L_)
    C, sigma, eps, seed = 3, 0.2, 0.0123, 991
    cur, gcur = _dev(0.3 * rs.randn(C, p)), _dev(5 * rs.randn(C, p))
    grads = [_dev(5 * rs.randn(C, p)) for _ in range(L_)]
    epsv = torch.full((C,), eps, dtype=F64, device="cuda")
    ones = torch.ones(C, p, dtype=F64, device="cuda")
    for f32 in (False, True):
        fixed = _one_step('fixed', cur, gcur, grads, sigma, eps, None, 4, seed, 6, f32)
        for scale in (None, ones):
            s = _one_step('s', cur, gcur, grads, sigma, epsv, scale, 4, seed, 6, f32)
            for beta in (None, torch.ones(C, dtype=F64, device="cuda")):
                got = _one_step('t', cur, gcur, grads, sigma, epsv, scale, 4, seed, 6, f32, beta=beta)
                for name, a, b, c in zip(("mom", "q", "kin_cur", "kin_prop"), got, fixed, s):
                    assert np.array_equal(a, b) and np.array_equal(a, c), (name, f32, scale is None, beta is None)
    assert np.all(fixed[2] > 0) and np.all(fixed[3] > 0)


def _close(got, ref, rtol):
    # elementwise relative; entries that cancelled to far below the array's scale are held to that scale
    np.testing.assert_allclose(got, ref, rtol=rtol, atol=1e-2 * rtol * np.abs(ref).max())


def test_one_step_equals_the_numpy_whitened_leapfrog_on_the_kernel_momenta():
    """C = 3 chains, three step sizes, a random positive scale: one trajectory (L = 3) of the kernels, fed the gradient
    kernel's gradients at the kernel's own positions, against the whitened leapfrog of the contract in numpy on the same
    momenta and gradients, to 1e-12; then the same with float32 gradients, exact on the rounded gradients and at float32
    accuracy against the float64 run."""
    dims, L_, sigma, seed, chain0, step = (1, 8, 8, 1), 3, 0.2, 77, 2, 9
    x, y = _problem(N=40)
    arch = MLPArch(dims, "tanh")
    op = BatchedMLP(arch, x, y)
    rs = np.random.RandomState(8)
    C, p = 3, arch.nparams
    ini = 0.3 * rs.randn(C, p)
    eps, scale = np.array([0.002, 0.0051, 0.0007]), np.exp(rs.randn(C, p))
    cur, epsd, scaled = _dev(ini), _dev(eps), _dev(scale)
    gs = -0.5 / sigma ** 2
    _, g0 = op.sse_grad(cur)
    g0 = g0.clone()
    # the N(0, I) draw itself: the begin kernel on a zero gradient
    z, _, kz, _ = _one_step('s', cur, torch.zeros_like(cur), [torch.zeros_like(cur)], sigma, epsd, scaled, chain0, seed, step)
    L = _lib.lib()
    nk = L.qn_hmc_parts(p)
    results = {}
    for f32 in (False, True):
        mom, q = torch.empty_like(cur), torch.empty_like(cur)
        kc, kp = torch.zeros(C, nk, dtype=F64, device="cuda"), torch.zeros(C, nk, dtype=F64, device="cuda")
        st = torch.tensor([step, 0], dtype=torch.int64, device="cuda")
        _lib.check(L.qn_hmc_begin_s(cur.data_ptr(), g0.data_ptr(), sigma, epsd.data_ptr(), scaled.data_ptr(), C, chain0, p, seed,
                                    st.data_ptr(), mom.data_ptr(), q.data_ptr(), kc.data_ptr(), None), "qn_hmc_begin_s")
        e, s = eps[:, None], scale
        u = z + (e / 2) * s * (gs * g0.cpu().numpy())
        qq = ini + e * s * u
        for j in range(L_):
            _, g = op.sse_grad(q)
            g = g.float() if f32 else g.clone()
            _lib.check(L.qn_hmc_leap_s(g.data_ptr(), _lib.QN_F32 if f32 else _lib.QN_F64, sigma, epsd.data_ptr(),
                                       scaled.data_ptr(), int(j == L_ - 1), C, p, mom.data_ptr(), q.data_ptr(), kp.data_ptr(),
                                       None), "qn_hmc_leap_s")
            gl = gs * g.double().cpu().numpy()
            if j != L_ - 1:
                u = u + e * s * gl
                qq = qq + e * s * u
            else:
                u = u + (e / 2) * s * gl
        torch.cuda.synchronize()
        _close(mom.cpu().numpy(), u, 1e-12)
        _close(q.cpu().numpy(), qq, 1e-12)
        np.testing.assert_allclose(0.5 * kc.cpu().numpy().sum(axis=1), 0.5 * (z ** 2).sum(axis=1), rtol=1e-12)
        np.testing.assert_allclose(0.5 * kp.cpu().numpy().sum(axis=1), 0.5 * (u ** 2).sum(axis=1), rtol=1e-12)
        results[f32] = (mom.cpu().numpy(), q.cpu().numpy())
    assert np.array_equal(kz, kc.cpu().numpy())
    # float32 gradients: relative rounding 6e-8 per gradient entry, L = 3 kicks
    _close(results[True][0], results[False][0], 1e-5)
    _close(results[True][1], results[False][1], 1e-5)
    assert not np.array_equal(results[True][0], results[False][0])


def test_adapt_kernel_equals_the_numpy_recurrences():
    """200 synthetic warm-up steps, states N(1, 1), acceptances in [0, 1] with NaN, 0 and values above 1, window ends at steps
    40 and 120 (collection from step 11, and again 121 .. 160 without an end, so the final moments are not zero): step
    sizes after every step, dual-averaging state, mean, M2 and scale against numpy to 1e-12 relative -- every update commits a
    few roundings of 1.1e-16 on O(1) quantities, so 200 updates stay below about 1e-13.  Chain 0 has NaN wherever chain 1 has
    0: their step sizes must be identical."""
    L = _lib.lib()
    C, p, nst, delta, eps0 = 3, 1101, 200, 0.8, 0.07                # p odd, two workgroups per chain
    assert L.qn_hmc_parts(p) == 2
    rs = np.random.RandomState(5)
    al = rs.rand(C, nst + 1)
    al[2, 5::7] = 1.0 + 3 * rs.rand(len(al[2, 5::7]))                # above 1 (counts as 1)
    al[2, 3], al[2, 50] = np.inf, 0.0
    al[1] = al[0]
    special = rs.rand(nst + 1) < 0.3
    al[0, special], al[1, special] = np.nan, 0.0
    X = 1.0 + rs.randn(nst + 1, C, p)
    ends, start, stop = (40, 120), 10, 160
    alphas, Xd = _dev(al), _dev(X)
    eps = torch.full((C,), eps0, dtype=F64, device="cuda")
    da = torch.zeros(C, 4, dtype=F64, device="cuda")
    da[:, 0] = np.log(10 * eps0)
    mean, m2 = torch.zeros(C, p, dtype=F64, device="cuda"), torch.zeros(C, p, dtype=F64, device="cuda")
    scale = torch.ones(C, p, dtype=F64, device="cuda")
    st = torch.zeros(2, dtype=torch.int64, device="cuda")
    hist = torch.zeros(nst + 1, C, dtype=F64, device="cuda")
    scales = {}
    # numpy side
    r_eps, r_mu = np.full(C, eps0), np.full(C, np.log(10 * eps0))
    r_hb, r_lb, r_le = np.zeros(C), np.zeros(C), np.zeros(C)
    r_mean, r_m2, r_scale = np.zeros((C, p)), np.zeros((C, p)), np.ones((C, p))
    r_hist, m, n, par = np.zeros((nst + 1, C)), 0, 0, 0
    for k in range(1, nst + 1):
        par ^= 1                                                      # the slot the accept call of step k wrote
        st[par] = k
        m += 1
        collect = start < k <= stop
        n = n + 1 if collect else 0
        finish, freeze = k in ends, k == nst
        _lib.check(L.qn_hmc_adapt(Xd[k].data_ptr(), alphas.data_ptr(), nst, st.data_ptr(), par, C, p, m, delta, int(collect),
                                  int(finish), int(freeze), n, da.data_ptr(), eps.data_ptr(), mean.data_ptr(), m2.data_ptr(),
                                  scale.data_ptr(), None), "qn_hmc_adapt")
        hist[k] = eps
        a = np.where(np.isnan(al[:, k]), 0.0, np.minimum(1.0, al[:, k]))
        r_hb = (1 - 1 / (m + 10)) * r_hb + (delta - a) / (m + 10)
        r_le = r_mu - np.sqrt(m) / 0.05 * r_hb
        eta = m ** -0.75
        r_lb = eta * r_le + (1 - eta) * r_lb
        r_eps = np.exp(r_lb if freeze else r_le)
        if collect:
            d = X[k] - r_mean
            r_mean = r_mean + d / n
            r_m2 = r_m2 + d * (X[k] - r_mean)
        if finish:
            r_scale = np.sqrt((n / (n + 5)) * r_m2 / (n - 1) + 1e-3 * 5 / (n + 5))
            scales[k] = (scale.clone(), r_scale)
            r_mean, r_m2, n = np.zeros((C, p)), np.zeros((C, p)), 0
            r_mu, r_hb, r_lb, m = np.log(10 * r_eps), np.zeros(C), np.zeros(C), 0
        r_hist[k] = r_eps
    torch.cuda.synchronize()
    h = hist.cpu().numpy()
    assert np.all(np.isfinite(h[1:])) and np.all(h[1:] > 0)
    np.testing.assert_allclose(h[1:], r_hist[1:], rtol=1e-12)
    assert np.array_equal(h[:, 0], h[:, 1])                           # NaN lowers the step exactly as a = 0 does
    assert h[1, 0] < eps0 * 10 and special[1:].any()
    np.testing.assert_allclose(da.cpu().numpy(), np.stack([r_mu, r_hb, r_lb, r_le], axis=1), rtol=1e-12)
    np.testing.assert_allclose(eps.cpu().numpy(), r_eps, rtol=1e-12)
    np.testing.assert_allclose(mean.cpu().numpy(), r_mean, rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(m2.cpu().numpy(), r_m2, rtol=1e-12)
    assert sorted(scales) == [40, 120] and np.abs(r_mean).max() > 0.5
    for k, (got, ref) in scales.items():
        np.testing.assert_allclose(got.cpu().numpy(), ref, rtol=1e-12)
    np.testing.assert_allclose(scale.cpu().numpy(), r_scale, rtol=1e-12)
    assert 0.7 < r_scale.mean() < 1.3                                 # states N(1, 1): a standard deviation near 1


def test_adapted_engine_samples_a_gaussian_posterior_from_a_diverging_step_size():
    """The linear-Gaussian model and the tolerances of test_gaussian_posterior_moments (test_gpu_device_hmc.py): from
    epsilon = 2 (posterior standard deviations are ~0.07: every fixed-step trajectory diverges, asserted on the unadapted
    engine) adapt = 200 warm-up steps must leave chains that accept and reproduce the posterior's mean and covariance."""
    rs = np.random.RandomState(1)
    N, sigma = 50, 0.5
    x = rs.randn(N, 1)
    y = 1.5 * x - 0.7 + sigma * rs.randn(N, 1)
    arch = MLPArch((1, 1), "identity")
    op = BatchedMLP(arch, x, y)
    A = np.hstack([x, np.ones((N, 1))])
    cov = sigma ** 2 * np.linalg.inv(A.T @ A)
    mean = np.linalg.solve(A.T @ A, A.T @ y).ravel()
    C, nwarm, nmcmc = 256, 200, 600
    ini = mean + 0.1 * rs.randn(C, 2)
    fixed = DeviceHMC(op, sigma, epsilon=2.0, L=8, seed=11).run(60, ini)
    assert fixed['accrate'].max().item() == 0.0 and 'epsilon' not in fixed
    r = DeviceHMC(op, sigma, epsilon=2.0, L=8, seed=11, adapt=nwarm).run(nmcmc, ini)
    eps = r['epsilon'].cpu().numpy()
    assert eps.shape == (C,) and np.all(np.isfinite(eps)) and np.all(eps > 0)
    assert r['nwarm'] == nwarm and r['mass_scale'].shape == (C, 2)
    sc = r['mass_scale'].cpu().numpy()
    assert np.all(np.isfinite(sc)) and np.all(sc > 0)
    post = r['chain'][:, nwarm + 100:]
    moved = (post[:, 1:] != post[:, :-1]).any(dim=2).double().mean().item()
    assert 0.6 < moved <= 1.0, moved
    ch = post.cpu().numpy().reshape(-1, 2)
    se = np.sqrt(np.diag(cov) / (C * 10))                              # generous: ~10 effective samples per chain
    assert np.all(np.abs(ch.mean(axis=0) - mean) < 5 * se)
    np.testing.assert_allclose(np.cov(ch.T), cov, rtol=0.15, atol=0.1 * np.abs(cov).max())


def _run(op, ini, nmcmc, **kw):
    return DeviceHMC(op, 0.2, epsilon=0.002, L=3, seed=9, adapt=30, **kw).run(nmcmc, ini)


def test_adapted_chains_do_not_depend_on_how_they_are_split():
    """Criteria of test_chains_do_not_depend_on_how_they_are_split, here with the warm-up's outputs: all adaptation state is
    per chain, so a chain's step size and scale do not depend on the launch it ran in."""
    x, y = _problem(N=64)
    arch = MLPArch((1, 16, 16, 1), "tanh")
    op = BatchedMLP(arch, x, y)
    C, nmcmc = 6, 60
    ini = np.stack([np.random.RandomState(50 + c).rand(arch.nparams) for c in range(C)])
    whole = _run(op, ini, nmcmc, chain0=0)
    a = _run(op, ini[:2], nmcmc, chain0=0)
    b = _run(op, ini[2:], nmcmc, chain0=2)
    two = _run(op, ini, nmcmc, chain0=0, groups=2)
    assert whole['nwarm'] == a['nwarm'] == two['nwarm'] == 30
    for k in ('chain', 'logpost', 'alphas', 'accrate', 'mapparams', 'maxpost', 'epsilon', 'mass_scale'):
        joined = torch.cat([a[k], b[k]]).cpu().numpy()
        # identical random numbers; only the summation order of a chain's SSE / gradient depends on the batch size
        np.testing.assert_allclose(joined, whole[k].cpu().numpy(), rtol=1e-7, atol=1e-9, err_msg=k)
        np.testing.assert_allclose(two[k].cpu().numpy(), whole[k].cpu().numpy(), rtol=1e-7, atol=1e-9, err_msg=k)
    moved = lambda r: (r['chain'][:, 1:] != r['chain'][:, :-1]).any(dim=2).cpu().numpy()
    assert np.array_equal(np.concatenate([moved(a), moved(b)]), moved(whole))
    assert 0.3 < whole['accrate'].mean().item() <= 1.0
    eps = whole['epsilon'].cpu().numpy()
    assert len(set(eps.tolist())) == C and not np.any(eps == 0.002)      # every chain found its own step size
    assert whole['mass_scale'].shape == (C, arch.nparams) and (whole['mass_scale'] != 1).all()


@pytest.mark.parametrize("nmcmc", [60, 61])
def test_adapted_graph_replay_equals_direct_launches_bit_for_bit(nmcmc):
    """The warm-up is launched directly either way; the sampling steps on the frozen arrays are replayed in pairs (odd
    remainder: the last step is launched directly)."""
    x, y = _problem(N=64)
    arch = MLPArch((1, 16, 16, 1), "tanh")
    op = BatchedMLP(arch, x, y)
    ini = np.stack([np.random.RandomState(70 + c).rand(arch.nparams) for c in range(6)])
    d = _run(op, ini, nmcmc)
    g = _run(op, ini, nmcmc, use_graph=True)
    assert set(d) == set(g) and d['nwarm'] == g['nwarm'] == 30
    for k in d:
        if k != 'nwarm':
            assert torch.equal(d[k], g[k]), (nmcmc, k)


def test_step_size_only_and_mala_engines():
    x, y = _problem(N=64)
    arch = MLPArch((1, 16, 16, 1), "tanh")
    op = BatchedMLP(arch, x, y)
    ini = np.stack([np.random.RandomState(90 + c).rand(arch.nparams) for c in range(4)])
    r = DeviceHMC(op, 0.2, epsilon=0.002, L=2, seed=3, adapt=40, adapt_mass=False).run(50, ini)
    assert r['mass_scale'] is None and r['nwarm'] == 40 and (r['epsilon'] > 0).all()
    eng = DeviceMALA(op, 0.2, epsilon=0.002, seed=3, adapt=40)
    assert eng.L == 1 and eng.target_accept == 0.574
    r = eng.run(50, ini)
    assert r['mass_scale'].shape == (4, arch.nparams) and torch.isfinite(r['epsilon']).all() and (r['epsilon'] > 0).all()
    with pytest.raises(ValueError):
        DeviceHMC(op, 0.2, adapt=10).run(5, ini)


@pytest.mark.parametrize("sampler", ["hmc", "mala"])
def test_solver_stores_the_adapted_step_size_and_scale(sampler):
    from quinn_amd.nns.mlp import MLP
    from quinn_amd.solvers.nn_mcmc import NN_MCMC
    x, y = _problem(seed=2, N=32)
    torch.manual_seed(0)
    s = NN_MCMC(MLP(1, 1, (8, 8), activ="tanh"), verbose=False)
    assert s.pdim == 97
    params = {"epsilon": 0.01, "adapt": 50}
    if sampler == "hmc":
        params["L"] = 3
    s.fit(x, y, zflag=False, datanoise=0.3, nmcmc=80, param_ini=0.1 * np.ones(s.pdim), sampler=sampler, sampler_params=params,
          nchains=4, seeds=[5, 6, 7, 8], engine="device")
    r = s.mcmc_results
    assert r['nwarm'] == 50 and r['epsilon'].shape == (4,) and r['mass_scale'].shape == (4, 97)
    assert np.all(np.isfinite(r['epsilon'])) and np.all(r['epsilon'] > 0) and np.all(r['mass_scale'] > 0)
    assert s.samples.shape == (4, 81, 97) and np.all(np.isfinite(s.samples))
