"""GPU: the Gauss-Newton curvature kinds of qn_mlp_curv, the linearised predictive qn_mlp_glm_predict (csrc/qn_glm.hip) and
NN_Laplace(la_type='ggn' | 'ggn_diag') / predict_glm, against float64 torch.func Jacobians on the host."""
import os
import warnings

import numpy as np
import pytest
import torch

from quinn_amd.ops import MLPArch, BatchedMLP
from test_glm_cpu import jac_autograd, torch_net

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
U = 2.0 ** -53


def gamma(n):
    """The standard bound n u / (1 - n u) of a length-n sum of products in any order."""
    return n * U / (1 - n * U)


ARCHS = [((1, 16, 16, 1), "tanh", True), ((3, 7, 2), "relu", True), ((2, 5, 70, 3), "tanh", False),
         ((16, 33, 4), "identity", True), ((4, 1, 9, 17, 8, 2), "tanh", True), ((5, 37, 21, 4), "relu", False)]


def _ggn_ref(arch, w, x):
    J = jac_autograd(arch, w, x).reshape(-1, arch.nparams)
    return J.T @ J


@pytest.mark.parametrize("dims,act,bias", ARCHS)
@pytest.mark.parametrize("N", [1, 63, 1000])
def test_ggn_vs_autograd(dims, act, bias, N):
    arch = MLPArch(dims, act, bias)
    rs = np.random.RandomState((sum(dims) * 131 + N) % 2 ** 31)
    x = rs.randn(N, dims[0])
    B = 3
    W = rs.randn(B, arch.nparams) / np.sqrt(max(dims))
    nb = max(1, (2 * N) // 3)
    rows = np.stack([rs.permutation(N)[:nb] for _ in range(B)]).astype(np.int32)
    op = BatchedMLP(arch, x, None, device="cuda:0")
    G = op.curvature(W, "ggn", row_idx=rows)
    D = op.curvature(W, "ggn_diag", row_idx=rows).cpu().numpy()
    assert torch.equal(G, G.mT)
    G = G.cpu().numpy()
    for b in range(B):
        ref = _ggn_ref(arch, W[b], x[rows[b]])
        scale = np.max(np.abs(ref))
        print("ggn", dims, N, b, np.max(np.abs(G[b] - ref)) / scale, np.max(np.abs(D[b] - np.diag(ref))) / scale)
        assert np.max(np.abs(G[b] - ref)) <= 1e-11 * scale
        assert np.max(np.abs(D[b] - np.diag(ref))) <= 1e-12 * scale
        assert np.max(np.abs(D[b] - np.diag(G[b]))) <= 1e-12 * scale


def test_ggn_symmetric_deterministic_batch_independent():
    arch = MLPArch((2, 40, 40, 2), "tanh")
    rs = np.random.RandomState(11)
    x = rs.randn(700, 2)
    W = rs.randn(3, arch.nparams) / 6
    op = BatchedMLP(arch, x, None, device="cuda:0")
    for kind in ("ggn", "ggn_diag"):
        a = op.curvature(W, kind)
        b = op.curvature(W, kind)
        assert torch.equal(a, b), kind
        alone = op.curvature(W[1:2], kind)
        assert torch.equal(alone[0], a[1]), kind
        if kind == "ggn":
            assert torch.equal(a, a.mT)


def test_ggn_additive_over_row_tiles():
    """Nb above one row tile (4096 rows): the sum of the matrices of two row subsets equals the matrix of all rows."""
    arch = MLPArch((3, 30, 30, 2), "tanh")
    rs = np.random.RandomState(21)
    N = 9001
    x = rs.randn(N, 3)
    W = rs.randn(1, arch.nparams) / 6
    op = BatchedMLP(arch, x, None, device="cuda:0")
    r = np.arange(N, dtype=np.int32)
    for kind in ("ggn", "ggn_diag"):
        H = op.curvature(W, kind)[0]
        H1 = op.curvature(W, kind, row_idx=r[None, :4500])[0]
        H2 = op.curvature(W, kind, row_idx=r[None, 4500:])[0]
        scale = torch.max(torch.abs(H)).item()
        assert torch.max(torch.abs(H - H1 - H2)).item() <= 1e-12 * scale, kind
    assert torch.equal(op.curvature(W, "ggn")[0], op.curvature(W, "ggn")[0].T)


def test_ggn_equals_exact_hessian_at_zero_residual():
    arch = MLPArch((2, 24, 24, 3), "tanh")
    rs = np.random.RandomState(5)
    N = 300
    x = rs.randn(N, 2)
    W = rs.randn(2, arch.nparams) / 5
    op = BatchedMLP(arch, x, None, device="cuda:0")
    op.use_exact_float64()
    for b in range(2):
        Y = op.predict(W[b:b + 1])[0]
        opb = BatchedMLP(arch, x, Y, device="cuda:0")
        H = opb.curvature(W[b:b + 1], "full")[0]
        G = opb.curvature(W[b:b + 1], "ggn")[0]
        scale = max(torch.max(torch.abs(H)).item(), torch.max(torch.abs(G)).item())
        print("zero-residual |H - G| / scale", torch.max(torch.abs(H - G)).item() / scale)
        assert torch.max(torch.abs(H - G)).item() <= 2e-11 * scale
        opp = BatchedMLP(arch, x, Y + 0.5, device="cuda:0")
        Hp = opp.curvature(W[b:b + 1], "full")[0]
        assert torch.equal(opp.curvature(W[b:b + 1], "ggn")[0], G)          # Y is not read
        assert torch.max(torch.abs(Hp - G)).item() > 1e-6 * scale


PSD_CASE = dict(dims=(2, 12, 12, 1), seed=3, N=40, wscale=0.8, yscale=3.0)


def psd_case():
    """tanh network with large residuals on Nb * o = 40 < p = 205 rows: the exact Hessian of the data term has negative
    eigenvalues there (checked with autograd when this case was chosen: min eigenvalue -3.7e2 against max 1.0e3)."""
    c = PSD_CASE
    arch = MLPArch(c["dims"], "tanh")
    rs = np.random.RandomState(c["seed"])
    x = rs.randn(c["N"], c["dims"][0])
    y = c["yscale"] * rs.randn(c["N"], 1)
    W = c["wscale"] * rs.randn(1, arch.nparams)
    return arch, x, y, W


def test_ggn_psd_where_exact_hessian_is_not():
    arch, x, y, W = psd_case()
    assert x.shape[0] * arch.dims[-1] < arch.nparams
    op = BatchedMLP(arch, x, y, device="cuda:0")
    H = op.curvature(W, "full")[0]
    G = op.curvature(W, "ggn")[0]
    ev = torch.linalg.eigvalsh(H)
    print("exact Hessian eigenvalues: min", ev.min().item(), "max", ev.max().item())
    assert ev.min().item() < 0
    sigma, sigma_p = 0.1, 1.0
    A = G / sigma ** 2 + torch.eye(arch.nparams, dtype=torch.float64, device=G.device) / sigma_p ** 2
    torch.linalg.cholesky(A)                                                # raises if not positive definite


def _check_glm(arch, W, x, Sig, mean, cov, chunk=512):
    """Every entry of cov [B, N, o, o] within (1e-11 + gamma_2p) (|J| |Sigma| |J|^T) of J Sigma J^T (host float64)."""
    p = arch.nparams
    tol = 1e-11 + gamma(2 * p)
    net = torch.func.vmap(torch_net(arch), in_dims=(None, 0))
    worst = 0.0
    for b in range(W.shape[0]):
        S = Sig[b] if Sig[b].ndim == 2 else None
        for n0 in range(0, x.shape[0], chunk):
            xs = x[n0:n0 + chunk]
            J = jac_autograd(arch, W[b], xs)                                # [n, o, p]
            if S is not None:
                T, Ta = J @ S, np.abs(J) @ np.abs(S)
            else:
                T, Ta = J * Sig[b], np.abs(J) * np.abs(Sig[b])
            ref = np.einsum("nkp,nlp->nkl", T, J)
            mag = np.einsum("nkp,nlp->nkl", Ta, np.abs(J))
            err = np.abs(cov[b, n0:n0 + chunk] - ref)
            worst = max(worst, float(np.max(err / (tol * mag + 1e-300))))
            assert np.all(err <= tol * mag), (b, n0, float(np.max(err / (mag + 1e-300))), tol)
            fref = net(torch.as_tensor(W[b]), torch.as_tensor(xs)).numpy()
            assert np.max(np.abs(mean[b, n0:n0 + chunk] - fref)) <= 1e-11 * max(np.max(np.abs(fref)), 1e-300)
    print("glm worst error / bound", worst)


def _spd(rs, p, B):
    out = []
    for _ in range(B):
        A = rs.randn(p, p) / np.sqrt(p)
        out.append(A @ A.T + 0.5 * np.eye(p))
    return np.stack(out)


GLM_CASES = [((1, 16, 16, 1), "tanh", True, 1), ((3, 7, 2), "relu", True, 77), ((2, 5, 70, 4), "tanh", False, 333),
             ((16, 33, 4), "identity", True, 130), ((4, 9, 17, 8, 2), "tanh", True, 65), ((2, 30, 1), "tanh", True, 4100)]


@pytest.mark.parametrize("dims,act,bias,N", GLM_CASES)
def test_glm_predict_vs_autograd(dims, act, bias, N):
    arch = MLPArch(dims, act, bias)
    p, o = arch.nparams, dims[-1]
    rs = np.random.RandomState((sum(dims) * 17 + N) % 2 ** 31)
    x = rs.randn(N, dims[0])
    B = 2
    W = rs.randn(B, p) / np.sqrt(max(dims))
    op = BatchedMLP(arch, rs.randn(3, dims[0]), None, device="cuda:0")
    op.use_exact_float64()
    for Sig in (_spd(rs, p, B), 0.1 + rs.rand(B, p)):
        mean, cov = op.glm_predict(W, Sig, x)
        assert mean.shape == (B, N, o) and cov.shape == (B, N, o, o)
        assert torch.equal(cov, cov.mT)
        m2, c2 = op.glm_predict(W, Sig, x)
        assert torch.equal(mean, m2) and torch.equal(cov, c2)
        m1, c1 = op.glm_predict(W[1:2], Sig[1:2], x)                        # a member alone
        assert torch.equal(m1[0], mean[1]) and torch.equal(c1[0], cov[1])
        pred = op.predict(W, x)
        assert torch.max(torch.abs(pred - mean)).item() <= 1e-11 * torch.max(torch.abs(pred)).item()
        _check_glm(arch, W, x, Sig, mean.cpu().numpy(), cov.cpu().numpy())
    mean0, cov0 = BatchedMLP(arch, x, None, device="cuda:0").glm_predict(W, Sig)      # x defaults to the stored rows
    assert torch.equal(cov0, cov)


def test_glm_predict_cfg2_size():
    """p = 8513 (the 3x64 tanh network), N = 4096, a dense SPD Sigma; the host reference in row chunks."""
    arch = MLPArch((1, 64, 64, 64, 1), "tanh")
    p = arch.nparams
    rs = np.random.RandomState(9)
    N = 4096
    x = rs.rand(N, 1) * 2 - 1
    W = rs.randn(1, p) / 8
    Sig = _spd(rs, p, 1)
    op = BatchedMLP(arch, x, None, device="cuda:0")
    mean, cov = op.glm_predict(W, Sig)
    _check_glm(arch, W, x, Sig, mean.cpu().numpy(), cov.cpu().numpy(), chunk=1024)


def _ufit_data():
    rs = np.random.RandomState(0)
    x = rs.rand(15, 1) * 2 * np.pi - np.pi
    y = np.sin(x) + 0.02 * rs.randn(15, 1)
    return x[:13], y[:13], x[13:], y[13:]


@pytest.mark.parametrize("la_type", ["ggn", "ggn_diag"])
def test_nn_laplace_ggn_end_to_end(la_type):
    from quinn_amd.nns.mlp import MLP
    from quinn_amd.solvers import NN_Laplace
    from quinn_amd.solvers.nn_laplace import glm_mixture
    torch.manual_seed(0)
    np.random.seed(0)
    xtrn, ytrn, xval, yval = _ufit_data()
    net = MLP(1, 1, (11, 11, 11), biasorno=True, activ='tanh').double()
    la = NN_Laplace(net, la_type=la_type, nens=3, dfrac=0.8, verbose=False)
    la.fit(xtrn, ytrn, val=[xval, yval], lrate=0.01, batch_size=2, nepochs=50, freq_out=1000)
    p = la.nparams
    assert len(la.means) == 3 and la.cov_mats[0].shape == (p, p)
    for j in range(3):                                                       # H = G / datanoise^2 + I / priorsigma^2, inverted
        HS = la.hessians[j] @ la.cov_mats[j] * la.cov_scale
        assert np.max(np.abs(HS - np.eye(p))) <= 1e-6
    xg = np.linspace(-np.pi, np.pi, 11)[:, None]
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        y = la.predict_ens(xg, nens=20)
        ym, yv, yc = la.predict_glm(xg, msc=2)
    assert y.shape == (20, 11, 1) and np.isfinite(y).all()
    assert ym.shape == (11, 1) and yv.shape == (11, 1) and yc.shape == (11, 1, 1)
    arch = la.arch
    tol = 1e-11 + gamma(2 * p)
    f, S, mag = [], [], []
    for j in range(3):
        J = jac_autograd(arch, la.means[j], xg)
        f.append(torch.func.vmap(torch_net(arch), in_dims=(None, 0))(torch.as_tensor(la.means[j]), torch.as_tensor(xg)).numpy())
        S.append(np.einsum("nkp,pq,nlq->nkl", J, la.cov_mats[j], J))
        mag.append(np.einsum("nkp,pq,nlq->nkl", np.abs(J), np.abs(la.cov_mats[j]), np.abs(J)))
    mref, cref = glm_mixture(np.array(f), np.array(S))
    bound = tol * np.mean(mag, axis=0) + 1e-11 * np.max(np.abs(f)) ** 2      # the members' bounds, and the means through f f^T
    print("predict_glm error / bound", np.max(np.abs(yc - cref) / bound))
    assert np.all(np.abs(yc - cref) <= bound)
    assert np.max(np.abs(ym - mref)) <= 1e-11 * np.max(np.abs(mref))
    assert np.array_equal(yv[:, 0], yc[:, 0, 0])
    _, yvn, _ = la.predict_glm(xg, msc=1, noise=True)
    assert np.allclose(yvn - yv, la.datanoise ** 2, rtol=0, atol=1e-12 * np.max(yvn))
    assert la.predict_glm(xg, msc=0)[1:] == (None, None)


STAT = dict(cov_scale=1.0e8, M=4000)


def test_glm_agrees_with_sampled_predictive_for_a_tight_posterior():
    """nens = 1, the posterior narrowed by cov_scale = 1e8 so that the network is linear across it: the variance of M = 4000
    sampled predictions agrees with the closed form within 5 sqrt(2 / (M - 1)) = 0.11 relative (five standard deviations of a
    variance estimate from M Gaussian draws).  The second-order term of the variance falls as 1 / cov_scale^2, the linear one
    as 1 / cov_scale: a numpy check with 2e5 draws of this (1, 8, 8, 1) tanh network when the case was chosen found up to
    0.8 relative at cov_scale = 1e4 (where the data pin the linear term down), 1e-2 at 1e6 and nothing above the 3e-3 Monte
    Carlo noise at 1e8."""
    from quinn_amd.nns.mlp import MLP
    from quinn_amd.solvers import NN_Laplace
    torch.manual_seed(1)
    np.random.seed(1)
    xtrn, ytrn, xval, yval = _ufit_data()
    net = MLP(1, 1, (8, 8), biasorno=True, activ='tanh').double()
    la = NN_Laplace(net, la_type='ggn', nens=1, dfrac=1.0, cov_scale=STAT["cov_scale"], verbose=False)
    la.fit(xtrn, ytrn, val=[xval, yval], lrate=0.01, batch_size=4, nepochs=100, freq_out=1000)
    xg = np.linspace(-np.pi, np.pi, 9)[:, None]
    M = STAT["M"]
    np.random.seed(2)
    ms, vs, _ = la.predict_mom_sample(xg, msc=1, nsam=M)
    mg, vg, _ = la.predict_glm(xg, msc=1)
    rel = np.abs(vs - vg) / vg
    print("sampled vs glm variance, relative:", rel.ravel(), "margin", 5 * np.sqrt(2 / (M - 1)))
    assert np.all(rel <= 5 * np.sqrt(2 / (M - 1)))


def test_predict_glm_full_type_warns_on_negative_variance():
    """la_type='full' works with predict_glm; an indefinite covariance gives negative variances, reported and not clipped."""
    from quinn_amd.nns.mlp import MLP
    from quinn_amd.solvers import NN_Laplace
    net = MLP(1, 1, (6,), biasorno=True, activ='tanh').double()
    la = NN_Laplace(net, la_type='full', nens=1, verbose=False)
    p = la.nparams
    rs = np.random.RandomState(0)
    la.means = [0.3 * rs.randn(p)]
    la.cov_mats = [-np.eye(p)]
    la._factors, la._cov_dev = [None], [None]
    with pytest.warns(RuntimeWarning, match="negative"):
        m, v, _ = la.predict_glm(np.linspace(-1, 1, 5)[:, None])
    assert np.all(v < 0)


def test_ex_ufit_laplace_ggn_runs():
    import importlib.util
    path = os.path.join(HERE, "..", "examples", "ex_ufit.py")
    spec = importlib.util.spec_from_file_location("ex_ufit_laplace_ggn", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    np.random.seed(0)
    torch.manual_seed(0)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        ymean, ystd, rmse = mod.main('laplace_ggn', quick=True, mlp=True)
    assert ymean.shape == (11,) and ystd.shape == (11,) and np.isfinite(ymean).all()
