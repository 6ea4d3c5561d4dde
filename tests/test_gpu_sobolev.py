"""GPU: the input Jacobian qn_mlp_input_jac and the derivative-informed loss qn_mlp_sobolev_fwdbwd (csrc/qn_sobolev.hip), GradLoss,
loss_fn='gradloss' training, predict_jac_* of the solvers and NN_MCMC with gradient observations, against torch float64
autograd on the host (helpers of test_sobolev_cpu.py)."""
import numpy as np
import pytest
import torch

from quinn_amd.ops import MLPArch, BatchedMLP
from quinn_amd.nns.nnfit import draw_perms
from test_sobolev_cpu import jac_x_autograd, sobolev_autograd, torch_net

pytestmark = pytest.mark.gpu

# the architecture list of test_gpu_glm.py
ARCHS = [((1, 16, 16, 1), "tanh", True), ((3, 7, 2), "relu", True), ((2, 5, 70, 3), "tanh", False),
         ((16, 33, 4), "identity", True), ((4, 1, 9, 17, 8, 2), "tanh", True), ((5, 37, 21, 4), "relu", False)]
WEIGHTS = [(1.0, 0.0), (0.0, 1.0), (1.0, 0.37)]


def _problem(dims, act, bias, N, B=3):
    arch = MLPArch(dims, act, bias)
    rs = np.random.RandomState((sum(dims) * 131 + N) % 2 ** 31)
    d, o = dims[0], dims[-1]
    x, y, g = rs.randn(N, d), rs.randn(N, o), rs.randn(N, o, d)
    W = rs.randn(B, arch.nparams) / np.sqrt(max(dims))
    nb = max(1, (2 * N) // 3)
    rows = np.stack([rs.permutation(N)[:nb] for _ in range(B)]).astype(np.int32)
    return arch, x, y, g, W, rows


@pytest.mark.parametrize("dims,act,bias", ARCHS)
@pytest.mark.parametrize("N", [1, 63, 1000])
def test_jacobian_vs_autograd(dims, act, bias, N):
    arch, x, y, g, W, rows = _problem(dims, act, bias, N)
    op = BatchedMLP(arch, x, y, device="cuda:0")
    J, P = op.input_jacobian(W, want_pred=True)
    assert J.shape == (3, N, dims[-1], dims[0]) and P.shape == (3, N, dims[-1])
    Jsub = op.input_jacobian(W[1:2], x[rows[1]])[0].cpu().numpy()
    J, P = J.cpu().numpy(), P.cpu().numpy()
    for b in range(3):
        pref, Jref = (t.numpy() for t in jac_x_autograd(arch, W[b], x))
        ej, ep = np.max(np.abs(J[b] - Jref)) / np.max(np.abs(Jref)), np.max(np.abs(P[b] - pref)) / np.max(np.abs(pref))
        print("jac", dims, N, b, ej, ep)
        assert ej <= 1e-12 and ep <= 1e-12
    assert np.array_equal(Jsub, J[1][rows[1]])                    # a row's Jacobian does not depend on the other rows


@pytest.mark.parametrize("dims,act,bias", ARCHS)
@pytest.mark.parametrize("N", [1, 63, 1000])
def test_value_and_gradient_vs_autograd(dims, act, bias, N):
    arch, x, y, g, W, rows = _problem(dims, act, bias, N)
    op = BatchedMLP(arch, x, y, device="cuda:0")
    op.set_grad_data(g)
    op.use_exact_float64()
    _, gsse_ref_op = op.sse_grad(W, row_idx=rows)
    for wv, wg in WEIGHTS:
        sse, gsse, grad = (t.cpu().numpy() for t in op.sobolev(W, wv, wg, row_idx=rows))
        sse0, gsse0, none = op.sobolev(W, wv, wg, row_idx=rows, want_grad=False)
        assert none is None and np.array_equal(sse0.cpu().numpy(), sse) and np.array_equal(gsse0.cpu().numpy(), gsse)
        for b in range(3):
            r = rows[b]
            sref, gref, dref = sobolev_autograd(arch, W[b], x[r], y[r], g[r], wv, wg)
            es, eg = abs(sse[b] - sref) / sref, abs(gsse[b] - gref) / gref
            ed = np.max(np.abs(grad[b] - dref)) / np.max(np.abs(dref))
            print("sobolev", dims, N, (wv, wg), b, es, eg, ed)
            assert es <= 1e-11 and eg <= 1e-11
            assert ed <= 1e-10
        if (wv, wg) == (1.0, 0.0):
            ref = gsse_ref_op.double().cpu().numpy()
            for b in range(3):
                e = np.max(np.abs(grad[b] - ref[b])) / np.max(np.abs(ref[b]))
                print("sobolev vs sse_grad", dims, N, b, e)
                assert e <= 1e-10


def test_deterministic_and_batch_independent():
    arch = MLPArch((3, 40, 40, 2), "tanh")
    rs = np.random.RandomState(11)
    x, y, g = rs.randn(700, 3), rs.randn(700, 2), rs.randn(700, 2, 3)
    W = rs.randn(3, arch.nparams) / 6
    op = BatchedMLP(arch, x, y, device="cuda:0")
    op.set_grad_data(g)
    a = op.sobolev(W, 1.0, 0.37)
    b = op.sobolev(W, 1.0, 0.37)
    alone = op.sobolev(W[1:2], 1.0, 0.37)
    for u, v, w1 in zip(a, b, alone):
        assert torch.equal(u, v)
        assert torch.equal(w1[0], u[1])
    Ja, Jb = op.input_jacobian(W), op.input_jacobian(W)
    assert torch.equal(Ja, Jb) and torch.equal(op.input_jacobian(W[1:2])[0], Ja[1])
    # chunking over B against max_workspace_bytes changes nothing
    small = BatchedMLP(arch, x, y, device="cuda:0", max_workspace_bytes=1)
    small.set_grad_data(g)
    for u, v in zip(a, small.sobolev(W, 1.0, 0.37)):
        assert torch.equal(u, v)
    assert torch.equal(small.input_jacobian(W), Ja)


def test_additive_over_row_tiles():
    """Nb above one row tile (2048 rows): the results of two half row sets add up to the result of all rows."""
    arch = MLPArch((3, 30, 30, 2), "tanh")
    rs = np.random.RandomState(21)
    N = 5001
    x, y, g = rs.randn(N, 3), rs.randn(N, 2), rs.randn(N, 2, 3)
    W = rs.randn(2, arch.nparams) / 6
    op = BatchedMLP(arch, x, y, device="cuda:0")
    op.set_grad_data(g)
    r = np.tile(np.arange(N, dtype=np.int32), (2, 1))
    full = op.sobolev(W, 1.0, 0.37)
    h1 = op.sobolev(W, 1.0, 0.37, row_idx=r[:, :2500])
    h2 = op.sobolev(W, 1.0, 0.37, row_idx=r[:, 2500:])
    for u, v1, v2 in zip(full, h1, h2):
        scale = torch.max(torch.abs(u)).item()
        err = torch.max(torch.abs(u - v1 - v2)).item()
        print("tiles", err / scale)
        assert err <= 1e-12 * scale
    sref, gref, dref = sobolev_autograd(arch, W[0], x, y, g, 1.0, 0.37)
    assert abs(full[0][0].item() - sref) <= 1e-11 * sref and abs(full[1][0].item() - gref) <= 1e-11 * gref
    assert np.max(np.abs(full[2][0].cpu().numpy() - dref)) <= 1e-10 * np.max(np.abs(dref))
    J = op.input_jacobian(W[:1])[0].cpu().numpy()
    Jref = jac_x_autograd(arch, W[0], x)[1].numpy()
    assert np.max(np.abs(J - Jref)) <= 1e-12 * np.max(np.abs(Jref))


def test_nan_weight_stays_in_its_member():
    arch = MLPArch((2, 20, 20, 1), "tanh")
    rs = np.random.RandomState(3)
    x, y, g = rs.randn(300, 2), rs.randn(300, 1), rs.randn(300, 2)
    W = rs.randn(3, arch.nparams) / 4
    op = BatchedMLP(arch, x, y, device="cuda:0")
    op.set_grad_data(g)
    clean = op.sobolev(W, 1.0, 0.5)
    Jclean = op.input_jacobian(W)
    Wn = W.copy()
    Wn[1, 7] = np.nan
    bad = op.sobolev(Wn, 1.0, 0.5)
    Jbad = op.input_jacobian(Wn)
    torch.cuda.synchronize()
    for u, v in zip(clean + (Jclean,), bad + (Jbad,)):
        assert torch.equal(u[0], v[0]) and torch.equal(u[2], v[2])
    assert not torch.isfinite(bad[0][1]) and not torch.isfinite(bad[1][1])
    assert not torch.isfinite(bad[2][1]).all() and not torch.isfinite(Jbad[1]).all()


def test_float32_and_missing_data_refused():
    arch = MLPArch((2, 8, 1), "tanh")
    x = np.zeros((4, 2))
    op32 = BatchedMLP(arch, x, None, device="cuda:0", dtype="float32")
    with pytest.raises(ValueError, match="float64"):
        op32.input_jacobian(np.zeros((1, arch.nparams)))
    op = BatchedMLP(arch, x, None, device="cuda:0")
    with pytest.raises(ValueError, match="set_grad_data"):
        op.sobolev(np.zeros((1, arch.nparams)), 1.0, 1.0)
    with pytest.raises(ValueError, match="gradient data of shape"):
        op.set_grad_data(np.zeros((3, 2)))


# ---------------------------------------------------------------- GradLoss
def test_gradloss_module():
    from quinn_amd.nns.losses import GradLoss
    torch.manual_seed(2)
    net = torch.nn.Sequential(torch.nn.Linear(2, 12), torch.nn.Tanh(), torch.nn.Linear(12, 1)).double()
    arch = MLPArch.from_module(net)
    rs = np.random.RandomState(8)
    x, y, g = rs.randn(40, 2), rs.randn(40, 1), rs.randn(40, 2)
    loss = GradLoss(net, lam=0.7, xtrn=x, gtrn=g)
    w = np.concatenate([p.detach().numpy().ravel() for p in net.parameters()])
    xb, yb = x[:13], y[:13]                                       # a minibatch: the penalty is still over all of xtrn
    wt = torch.tensor(w, requires_grad=True)
    pred = torch.func.vmap(torch_net(arch), in_dims=(None, 0))(wt, torch.as_tensor(xb))
    J = jac_x_autograd(arch, wt, x)[1]
    ref = ((pred - torch.as_tensor(yb)) ** 2).mean() + 0.7 * ((J[:, 0, :] - torch.as_tensor(g)) ** 2).mean()
    dref, = torch.autograd.grad(ref, wt)
    val, grad = loss.value_and_grad(w, xb, yb, want_grad=True)
    assert abs(val - ref.item()) <= 1e-11 * abs(ref.item())
    assert np.max(np.abs(grad - dref.numpy())) <= 1e-10 * np.max(np.abs(dref.numpy()))
    assert abs(loss(torch.as_tensor(xb), torch.as_tensor(yb)).item() - ref.item()) <= 1e-11 * abs(ref.item())


# ---------------------------------------------------------------- training
def _fxy(x):
    y = (np.sin(x[:, 0]) * x[:, 1])[:, None]
    g = np.stack([np.cos(x[:, 0]) * x[:, 1], np.sin(x[:, 0])], axis=1)
    return y, g


def _ens_net():
    torch.manual_seed(5)
    return torch.nn.Sequential(torch.nn.Linear(2, 16), torch.nn.Tanh(), torch.nn.Linear(16, 16), torch.nn.Tanh(),
                               torch.nn.Linear(16, 1)).double()


def test_ens_gradloss_training_matches_torch_loop():
    from quinn_amd.solvers.nn_ens import NN_Ens
    rs = np.random.RandomState(4)
    N, nens, nepochs, lam, lrate, bs = 24, 4, 300, 0.5, 0.01, 8
    x = rs.uniform(-2, 2, (N, 2))
    y, g = _fxy(x)
    xt = rs.uniform(-2, 2, (200, 2))
    yt, gt = _fxy(xt)
    net = _ens_net()
    arch = MLPArch.from_module(net)
    w0 = np.concatenate([p.detach().numpy().ravel() for p in net.parameters()])

    def fit(lam_):
        np.random.seed(10)
        torch.manual_seed(20)
        ens = NN_Ens(net, nens=nens, dfrac=0.75)
        ens.fit(x, y, loss_fn='gradloss', gtrn=g, lam=lam_, nepochs=nepochs, lrate=lrate, batch_size=bs)
        return ens

    ens = fit(lam)
    # the same draws, consumed in the same order, for the host loop
    np.random.seed(10)
    torch.manual_seed(20)
    ntrn = int(N * 0.75)
    rows = np.stack([np.random.permutation(N)[:ntrn] for _ in range(nens)])
    perms = draw_perms(nens, nepochs, ntrn)
    f = torch_net(arch)
    xT, yT, gT = torch.as_tensor(x), torch.as_tensor(y), torch.as_tensor(g)

    def loss_of(w, r_val, r_pen):
        pred = torch.func.vmap(f, in_dims=(None, 0))(w, xT[r_val])
        J = torch.func.vmap(torch.func.jacrev(f, argnums=1), in_dims=(None, 0))(w, xT[r_pen])
        return ((pred - yT[r_val]) ** 2).mean() + lam * ((J[:, 0, :] - gT[r_pen]) ** 2).mean()

    worst = 0.0
    for j in range(nens):
        w = torch.tensor(w0, requires_grad=True)
        opt = torch.optim.Adam([w], lr=lrate)
        hist = np.asarray(ens.learners[j].history)
        rj = torch.as_tensor(rows[j])
        upd = 0
        for t in range(nepochs):
            for i in range(0, ntrn, bs):
                rb = rj[torch.as_tensor(perms[j, t, i:i + bs])]
                loss = loss_of(w, rb, rj)
                with torch.no_grad():
                    lval = loss_of(w.detach(), rj, rj).item()      # no validation set: the member's own rows
                for col, ref in ((1, loss.item()), (3, lval)) + (((2, lval),) if i == 0 else ()):
                    worst = max(worst, abs(hist[upd, col] - ref) / abs(ref))
                opt.zero_grad()
                loss.backward()
                opt.step()
                upd += 1
        assert upd == hist.shape[0]
    print("gradloss training: worst relative history difference", worst)
    assert worst <= 1e-8

    # against the same members trained on values only: smaller gradient error on held-out points
    ens0 = fit(0.0)
    op = BatchedMLP(arch, xt, yt, device="cuda:0")
    op.set_grad_data(gt)
    _, gs, _ = op.sobolev(ens.fit_results['final_w'], 0.0, 1.0, want_grad=False)
    _, gs0, _ = op.sobolev(ens0.fit_results['final_w'], 0.0, 1.0, want_grad=False)
    print("held-out gsse with / without the penalty", gs.cpu().numpy(), gs0.cpu().numpy())
    assert bool((gs < gs0).all())


def test_nnfit_gradloss_single_module():
    from quinn_amd.nns.nnfit import nnfit
    rs = np.random.RandomState(6)
    x = rs.uniform(-2, 2, (30, 2))
    y, g = _fxy(x)
    net = _ens_net()
    torch.manual_seed(1)
    info = nnfit(net, x, y, loss_fn='gradloss', lossparams={'gtrn': g, 'lam': 1.0}, nepochs=50, lrate=0.01, freq_out=1000)
    h = np.asarray(info['history'])
    assert h.shape == (50, 4) and np.isfinite(h).all() and h[-1, 1] < h[0, 1]
    assert np.allclose(h[:, 1], h[:, 3], rtol=1e-12)              # full batch, no validation set: the same loss


# ---------------------------------------------------------------- prediction
def _check_jac_predictions(solver, W, x, **ens_args):
    arch = solver.arch
    st = np.random.get_state()
    before = solver.predict_ens(x, **ens_args)
    np.random.set_state(st)
    J = solver.predict_jac_ens(x, **ens_args)
    assert J.shape == (W.shape[0], x.shape[0], arch.dims[-1], arch.dims[0])
    for m in range(W.shape[0]):
        Jref = jac_x_autograd(arch, W[m], x)[1].numpy()
        assert np.max(np.abs(J[m] - Jref)) <= 1e-12 * np.max(np.abs(Jref))
    np.random.set_state(st)
    nsam = ens_args.pop('nens')
    mean, var = solver.predict_jac_mom_sample(x, msc=1, nsam=nsam, **ens_args)
    assert np.max(np.abs(mean - J.mean(0))) <= 1e-13 * np.max(np.abs(J))
    assert np.max(np.abs(var - J.var(0, ddof=1))) <= 1e-12 * np.max(J.var(0, ddof=1))
    np.random.set_state(st)
    mean0, var0 = solver.predict_jac_mom_sample(x, msc=0, nsam=nsam, **ens_args)
    assert var0 is None and np.array_equal(mean0, mean)
    np.random.set_state(st)
    assert np.array_equal(solver.predict_ens(x, nens=nsam, **ens_args), before)


def test_predict_jac_ens_nn_ens():
    from quinn_amd.solvers.nn_ens import NN_Ens
    rs = np.random.RandomState(12)
    x = rs.uniform(-2, 2, (20, 2))
    y, _ = _fxy(x)
    np.random.seed(3)
    torch.manual_seed(3)
    ens = NN_Ens(_ens_net(), nens=5)
    ens.fit(x, y, nepochs=20, lrate=0.01)
    np.random.seed(77)
    order = np.random.permutation(5)
    np.random.seed(77)
    _check_jac_predictions(ens, ens._best_w[order], rs.randn(17, 2), nens=5)


def _mcmc_problem():
    rs = np.random.RandomState(15)
    x = rs.uniform(-2, 2, (25, 2))
    y, g = _fxy(x)
    torch.manual_seed(9)
    net = torch.nn.Sequential(torch.nn.Linear(2, 6), torch.nn.Tanh(), torch.nn.Linear(6, 1)).double()
    return net, x, y, g


def test_mcmc_with_gradient_observations():
    from quinn_amd.solvers.nn_mcmc import NN_MCMC
    net, x, y, g = _mcmc_problem()
    s = NN_MCMC(net, verbose=False)
    arch, p = s.arch, s.pdim
    sig, sg = 0.3, 0.4
    rs = np.random.RandomState(2)
    ini = rs.randn(2, p) / 3
    s.fit(x, y, zflag=False, datanoise=sig, nmcmc=200, param_ini=ini, sampler='hmc', seeds=[1, 2],
          sampler_params={'epsilon': 0.01, 'L': 3}, gtrn=g, gradnoise=sg)
    lps = np.asarray(s.mcmc_results['logpost'])
    print("hmc with gradient data: acceptance", s.mcmc_results['accrate'])
    assert np.isfinite(lps).all() and np.all(np.asarray(s.mcmc_results['accrate']) > 0)
    assert s.samples.shape == (2, 201, p)
    # log-posterior and its gradient against autograd
    W = rs.randn(3, p) / 3
    lp, dlp = s.logpost_batch(W), s.logpostgrad_batch(W)
    N, o, d = x.shape[0], 1, 2
    for b in range(3):
        sref, gref, dref = sobolev_autograd(arch, W[b], x, y, g[:, None, :], -0.5 / sig ** 2, -0.5 / sg ** 2)
        ref = -0.5 * sref / sig ** 2 - 0.5 * gref / sg ** 2 - N * o * (np.log(sig) + 0.5 * np.log(2 * np.pi)) \
            - N * o * d * (np.log(sg) + 0.5 * np.log(2 * np.pi))
        assert abs(lp[b] - ref) <= 1e-11 * abs(ref)
        assert np.max(np.abs(dlp[b] - dref)) <= 1e-10 * np.max(np.abs(dref))
        assert abs(s.logpost(W[b], s.lpinfo) - lp[b]) == 0.0
    with pytest.raises(NotImplementedError, match="engine='host'"):
        s.fit(x, y, zflag=False, datanoise=sig, nmcmc=10, param_ini=ini[0], sampler='hmc', engine='device',
              sampler_params={'epsilon': 0.01, 'L': 3}, gtrn=g, gradnoise=sg)
    # predictions of the chain
    s.fit(x, y, zflag=False, datanoise=sig, nmcmc=200, param_ini=ini, sampler='hmc', seeds=[1, 2],
          sampler_params={'epsilon': 0.01, 'L': 3}, gtrn=g, gradnoise=sg)
    rows = [100 + j * 10 for j in range(10)]
    _check_jac_predictions(s, s.samples[1][rows], rs.randn(11, 2), nens=10, nburn=100, chain=1)
