"""GPU: the Kronecker-factored Gauss-Newton kernels (csrc/qn_kron.hip) -- factors, linearised predictive, sampler -- and
NN_Laplace(la_type='kron'), against the numpy restatement of test_kron_cpu.py and the existing Gauss-Newton kernels."""
import os
import warnings

import numpy as np
import pytest
import torch

from quinn_amd.ops import MLPArch, BatchedMLP, kron_sample
from test_glm_cpu import jac_np
from test_gpu_glm import GLM_CASES, STAT, _ufit_data, gamma
from test_kron_cpu import (kron_shapes, kron_factors_np, kron_eig_np, kron_dinv_np, kron_block_idx, kron_dense_cov_np,
                           kron_dense_prec_np, kron_glm_np, kron_sample_np)

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

ARCHS = [((1, 16, 16, 1), "tanh", True), ((3, 7, 2), "relu", True), ((2, 5, 70, 3), "tanh", False),
         ((16, 33, 4), "identity", True), ((4, 1, 9, 17, 8, 2), "tanh", True), ((2, 130, 1), "tanh", True)]


@pytest.mark.parametrize("dims,act,bias", ARCHS)
@pytest.mark.parametrize("N", [1, 63, 1000])
def test_kron_factors_vs_numpy(dims, act, bias, N):
    arch = MLPArch(dims, act, bias)
    rs = np.random.RandomState((sum(dims) * 131 + N) % 2 ** 31)
    x = rs.randn(N, dims[0])
    B = 3
    W = rs.randn(B, arch.nparams) / np.sqrt(max(dims))
    nb = max(1, (2 * N) // 3)
    rows = np.stack([rs.permutation(N)[:nb] for _ in range(B)]).astype(np.int32)
    op = BatchedMLP(arch, x, None, device="cuda:0")
    A, S, lay = op.kron_factors(W, row_idx=rows)
    assert A.shape == (B, lay.lenA) and S.shape == (B, lay.lenS)
    for b in range(B):
        Ar, Sr = kron_factors_np(arch, W[b], x[rows[b]])
        for i in range(len(dims) - 1):
            Ai, Si = lay.A(A[b], i), lay.S(S[b], i)
            assert torch.equal(Ai, Ai.T) and torch.equal(Si, Si.T)
            for got, ref in ((Ai.cpu().numpy(), Ar[i]), (Si.cpu().numpy(), Sr[i])):
                err = np.max(np.abs(got - ref)) / np.max(np.abs(ref))
                print("kron factors", dims, N, b, i, err)
                assert err <= 1e-11


@pytest.mark.parametrize("dims", [(2, 512, 1), (1, 256, 256, 1)])
def test_kron_factors_wide_layers(dims):
    """The widest layer the kernels take and a 256 x 257 layer block: 64 x 64 tiles off the diagonal, several per row."""
    arch = MLPArch(dims, "tanh")
    rs = np.random.RandomState(sum(dims))
    N, B = 63, 2
    x = rs.randn(N, dims[0])
    W = rs.randn(B, arch.nparams) / np.sqrt(max(dims))
    A, S, lay = BatchedMLP(arch, x, None, device="cuda:0").kron_factors(W)
    for b in range(B):
        Ar, Sr = kron_factors_np(arch, W[b], x)
        for i in range(len(dims) - 1):
            Ai, Si = lay.A(A[b], i), lay.S(S[b], i)
            assert torch.equal(Ai, Ai.T) and torch.equal(Si, Si.T)
            for got, ref in ((Ai.cpu().numpy(), Ar[i]), (Si.cpu().numpy(), Sr[i])):
                assert np.max(np.abs(got - ref)) <= 1e-11 * np.max(np.abs(ref))


def test_kron_factors_deterministic_batch_independent_additive():
    arch = MLPArch((2, 40, 40, 2), "tanh")
    rs = np.random.RandomState(11)
    x = rs.randn(700, 2)
    W = rs.randn(3, arch.nparams) / 6
    op = BatchedMLP(arch, x, None, device="cuda:0")
    A, S, _ = op.kron_factors(W)
    A2, S2, _ = op.kron_factors(W)
    assert torch.equal(A, A2) and torch.equal(S, S2)
    A1, S1, _ = op.kron_factors(W[1:2])
    assert torch.equal(A1[0], A[1]) and torch.equal(S1[0], S[1])
    # more rows than one row tile: the factors of two row subsets add up to the factors of all rows
    arch = MLPArch((3, 30, 30, 2), "tanh")
    rs = np.random.RandomState(21)
    N = 9001
    x = rs.randn(N, 3)
    W = rs.randn(1, arch.nparams) / 6
    op = BatchedMLP(arch, x, None, device="cuda:0")
    r = np.arange(N, dtype=np.int32)
    full = op.kron_factors(W)
    lo = op.kron_factors(W, row_idx=r[None, :4500])
    hi = op.kron_factors(W, row_idx=r[None, 4500:])
    for q in range(2):
        scale = torch.max(torch.abs(full[q])).item()
        assert torch.max(torch.abs(full[q] - lo[q] - hi[q])).item() <= 1e-12 * scale


def test_kron_blocks_vs_ggn_kernel():
    dims = (2, 24, 24, 3)
    arch = MLPArch(dims, "tanh")
    rs = np.random.RandomState(5)
    N = 300
    x = rs.randn(N, 2)
    W = rs.randn(1, arch.nparams) / 5
    op = BatchedMLP(arch, x, None, device="cuda:0")
    L = len(dims) - 1
    G = op.curvature(W, "ggn")[0].cpu().numpy()
    A, S, lay = op.kron_factors(W)
    idx = kron_block_idx(arch, L - 1)                                          # the last layer's block is exact at every Nb
    blk = np.kron(lay.S(S[0], L - 1).cpu().numpy(), lay.A(A[0], L - 1).cpu().numpy()) / N
    assert np.max(np.abs(blk - G[np.ix_(idx, idx)])) <= 1e-11 * np.max(np.abs(G))
    one = np.array([[17]], dtype=np.int32)                                     # one row: every layer block is exact
    G = op.curvature(W, "ggn", row_idx=one)[0].cpu().numpy()
    A, S, lay = op.kron_factors(W, row_idx=one)
    for i in range(L):
        idx = kron_block_idx(arch, i)
        blk = np.kron(lay.S(S[0], i).cpu().numpy(), lay.A(A[0], i).cpu().numpy())
        assert np.max(np.abs(blk - G[np.ix_(idx, idx)])) <= 1e-11 * np.max(np.abs(G))


def _random_posterior(arch, rs, B):
    """Per member random SPD factors A A^T + 0.5 I per layer, their eigendecompositions and the pair variances: (per-member
    lists US, UA, Dinv) and the packed arrays UA [B, lenA], US [B, lenS], Dinv [B, p] (kron order), Dih."""
    e, h, offK, perm = kron_shapes(arch)
    spd = lambda n: (lambda a: a @ a.T + 0.5 * np.eye(n))(rs.randn(n, n) / np.sqrt(n))      # noqa: E731
    mem = []
    for _ in range(B):
        lamS, US = kron_eig_np([spd(n) for n in h])
        lamA, UA = kron_eig_np([spd(n) for n in e])
        mem.append((US, UA, kron_dinv_np(lamS, lamA, 7, 0.5, 1.0, 1.0)))
    pack = lambda q: np.stack([np.concatenate([v.reshape(-1) for v in m[q]]) for m in mem])   # noqa: E731
    return mem, pack(1), pack(0), pack(2)


def kron_glm_m(arch):
    """Length of the longest summation chain behind one entry of qn_mlp_kron_glm_predict's covariance (see
    test_kron_glm_predict)."""
    e, h, _, _ = kron_shapes(arch)
    return 3 * max(e) + 2 * max(h) + sum((v + 63) // 64 for v in h) + 11


# (2, 512, 1): the widest layer the kernels take (the sampler's LDS panel is 64 KB there); (1, 256, 256, 1): a 256 x 257 layer
# block, p = 66 561 -- the widths of the networks the type is meant for
KRON_GLM_CASES = GLM_CASES + [((2, 130, 1), "tanh", True, 50), ((2, 512, 1), "tanh", True, 20),
                              ((1, 256, 256, 1), "tanh", True, 20)]


@pytest.mark.parametrize("dims,act,bias,N", KRON_GLM_CASES)
def test_kron_glm_predict(dims, act, bias, N):
    """Bound per entry: (1e-11 + gamma_m) mag, mag the formula evaluated with |U_S|, |U_A|, |g|, |~in|.  The chain m of the
    kernel, with e = max e_i and h = max h_{i+1}: a term Dinv ah_c^2 gh^k_a gh^l_a carries the rotation ah twice (each an e-term
    MFMA sum: 2 e) and its square (1), the sum over c of T (e products and additions), gh^k and gh^l (h-term sums: 2 h), the two
    products with them (2), the sum over the 64 units of a tile (4 fused multiply-adds and a 4-step butterfly: 8) and one
    addition per tile of 64 units of every layer (sum_i ceil(h_{i+1} / 64)): m = 3 e + 2 h + sum_i ceil(h_{i+1} / 64) + 11.
    Above p = 16384 no dense Sigma exists: the reference is then the numpy formula itself, which test_kron_cpu.py ties to
    J Sigma J^T.  The 1e-11 covers the per-row forward / backward pass, as in test_gpu_glm.py."""
    arch = MLPArch(dims, act, bias)
    p, o = arch.nparams, dims[-1]
    rs = np.random.RandomState((sum(dims) * 17 + N) % 2 ** 31)
    x = rs.randn(N, dims[0])
    B = 2
    W = rs.randn(B, p) / np.sqrt(max(dims))
    mem, UA, US, Dinv = _random_posterior(arch, rs, B)
    op = BatchedMLP(arch, rs.randn(3, dims[0]), None, device="cuda:0")
    op.use_exact_float64()
    mean, cov = op.kron_glm_predict(W, UA, US, Dinv, x)
    assert mean.shape == (B, N, o) and cov.shape == (B, N, o, o)
    assert torch.equal(cov, cov.mT)
    m2, c2 = op.kron_glm_predict(W, UA, US, Dinv, x)
    assert torch.equal(mean, m2) and torch.equal(cov, c2)
    m1, c1 = op.kron_glm_predict(W[1:2], UA[1:2], US[1:2], Dinv[1:2], x)       # a member alone
    assert torch.equal(m1[0], mean[1]) and torch.equal(c1[0], cov[1])
    pred = op.predict(W, x)
    assert torch.max(torch.abs(pred - mean)).item() <= 1e-11 * torch.max(torch.abs(pred)).item()
    tol = 1e-11 + gamma(kron_glm_m(arch))
    covn = cov.cpu().numpy()
    dense = p <= 16384
    if dense:
        Sig = np.stack([kron_dense_cov_np(arch, *mem[b]) for b in range(B)])
        cdense = op.glm_predict(W, Sig, x)[1].cpu().numpy()                    # the dense kernel on the same posterior
    worst = 0.0
    for b in range(B):
        if dense:
            _, J = jac_np(arch, W[b], x)
            ref = np.einsum("nkp,pq,nlq->nkl", J, Sig[b], J)
        else:
            ref = kron_glm_np(arch, W[b], x, *mem[b])[1]
        _, mag = kron_glm_np(arch, W[b], x, *mem[b], absolute=True)
        err = np.abs(covn[b] - ref)
        worst = max(worst, float(np.max(err / (tol * mag + 1e-300))))
        assert np.all(err <= tol * mag), (b, float(np.max(err / (mag + 1e-300))), tol)
        if dense:
            magd = np.einsum("nkp,pq,nlq->nkl", np.abs(J), np.abs(Sig[b]), np.abs(J))
            assert np.all(np.abs(covn[b] - cdense[b]) <= tol * mag + (1e-11 + gamma(2 * p)) * magd)
    print("kron glm worst error / bound", dims, worst)


@pytest.mark.parametrize("dims,act,bias,N", KRON_GLM_CASES)
def test_kron_sample_vs_numpy(dims, act, bias, N):
    """Bound per entry: 1e-12 max|W_out - mean| plus gamma_{e + h + 4} times the formula with absolute values: the two rotations
    are an e-term and an h-term MFMA sum, plus the product Z Dih and the final addition of the mean."""
    arch = MLPArch(dims, act, bias)
    p = arch.nparams
    e, h, _, _ = kron_shapes(arch)
    rs = np.random.RandomState(sum(dims) * 29)
    B, js = 2, np.array([1, 0, 1, 1, 0])
    M = len(js)
    mem, UA, US, Dinv = _random_posterior(arch, rs, B)
    mean, Z = rs.randn(B, p), rs.randn(M, p)
    dev = torch.device("cuda:0")
    t = lambda a: torch.as_tensor(a, device=dev).contiguous()                  # noqa: E731
    out = kron_sample(arch, t(mean), t(UA), t(US), t(np.sqrt(Dinv)), js, Z)
    assert out.shape == (M, p)
    assert torch.equal(out, kron_sample(arch, t(mean), t(UA), t(US), t(np.sqrt(Dinv)), js, Z))
    out = out.cpu().numpy()
    g = gamma(max(e) + max(h) + 4)
    for m in range(M):
        US_, UA_, Dinv_ = mem[js[m]]
        Dih = [np.sqrt(d) for d in Dinv_]
        ref = kron_sample_np(arch, mean[js[m]], US_, UA_, Dih, Z[m])
        mag = kron_sample_np(arch, mean[js[m]], US_, UA_, Dih, Z[m], absolute=True) + np.abs(mean[js[m]])
        bound = 1e-12 * np.max(np.abs(out[m] - mean[js[m]])) + g * mag
        assert np.all(np.abs(out[m] - ref) <= bound), (m, float(np.max(np.abs(out[m] - ref) / bound)))


def _kron_np(k):
    """(S, A, US, UA, Dinv) per-layer numpy lists of one entry of NN_Laplace.kron."""
    return tuple([v.cpu().numpy() for v in k[key]] for key in ("S", "A", "US", "UA", "Dinv"))


def test_nn_laplace_kron_end_to_end():
    from quinn_amd.nns.mlp import MLP
    from quinn_amd.solvers import NN_Laplace
    from quinn_amd.solvers.nn_laplace import glm_mixture
    torch.manual_seed(0)
    np.random.seed(0)
    xtrn, ytrn, xval, yval = _ufit_data()
    net = MLP(1, 1, (11, 11, 11), biasorno=True, activ='tanh').double()
    la = NN_Laplace(net, la_type='kron', nens=3, dfrac=0.8, verbose=False)
    la.fit(xtrn, ytrn, val=[xval, yval], lrate=0.01, batch_size=2, nepochs=50, freq_out=1000)
    p, arch = la.nparams, la.arch
    assert len(la.means) == 3 and len(la.kron) == 3
    for j in range(3):
        S, A, US, UA, Dinv = _kron_np(la.kron[j])
        H = kron_dense_prec_np(arch, S, A, la.kron[j]["nb"], la.datanoise, la.priorsigma, la.cov_scale)
        cov = la.dense_cov(j)
        assert cov.shape == (p, p)
        assert np.max(np.abs(H @ cov - np.eye(p))) <= 1e-6
    xg = np.linspace(-np.pi, np.pi, 11)[:, None]
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        y = la.predict_ens(xg, nens=20)
        ym, yv, yc = la.predict_glm(xg, msc=2)
    assert y.shape == (20, 11, 1) and np.isfinite(y).all()
    assert la.predict_sample(xg).shape == (11, 1)
    assert ym.shape == (11, 1) and yv.shape == (11, 1) and yc.shape == (11, 1, 1)
    tol = 1e-11 + gamma(kron_glm_m(arch))
    f, C, mag = [], [], []
    for j in range(3):
        S, A, US, UA, Dinv = _kron_np(la.kron[j])
        fj, cj = kron_glm_np(arch, la.means[j], xg, US, UA, Dinv)
        f.append(fj), C.append(cj), mag.append(kron_glm_np(arch, la.means[j], xg, US, UA, Dinv, absolute=True)[1])
    mref, cref = glm_mixture(np.array(f), np.array(C))
    # the members' bounds, plus what the means' own 1e-11 relative error d_b does through the mixture's f f^T - mean mean^T:
    # to first order avg_b (d_b (f_b - mean)^T + (f_b - mean) d_b^T), |d_b| <= 1e-11 max|f|; and the mixture's own float64
    # arithmetic on numbers of size max|f|^2 (two products, a mean of three, a subtraction: 8 roundings)
    fa = np.array(f)
    dev = np.mean(np.abs(fa - mref), axis=0)                                   # [N, o]
    bound = tol * np.mean(mag, axis=0) + 1e-11 * np.max(np.abs(fa)) * (dev[:, :, None] + dev[:, None, :]) \
        + 8 * 2.0 ** -53 * np.max(np.abs(fa)) ** 2
    print("kron predict_glm error / bound", np.max(np.abs(yc - cref) / bound))
    assert np.all(np.abs(yc - cref) <= bound)
    assert np.max(np.abs(ym - mref)) <= 1e-11 * np.max(np.abs(mref))
    assert np.array_equal(yv[:, 0], yc[:, 0, 0])
    _, yvn, _ = la.predict_glm(xg, msc=1, noise=True)
    assert np.allclose(yvn - yv, la.datanoise ** 2, rtol=0, atol=1e-12 * np.max(yvn))
    assert la.predict_glm(xg, msc=0)[1:] == (None, None)
    # la_calc: the per-batch factor sums add up to the factors of all rows
    learner = la.learners[0]
    whole = la.la_calc(learner, xtrn, ytrn)
    parts = la.la_calc(learner, xtrn, ytrn, batch_size=4)
    assert len(la.means) == 5 and whole["nb"] == parts["nb"] == len(xtrn)
    for key in ("A", "S"):
        for a, b in zip(whole[key], parts[key]):
            assert torch.max(torch.abs(a - b)).item() <= 1e-12 * torch.max(torch.abs(a)).item()


def test_kron_where_the_dense_types_are_refused():
    """MLP(1, 1, (128, 128)): p = 16 897 > 16 384.  'ggn' refuses; 'kron' fits, predicts and never allocates p^2 numbers."""
    from quinn_amd import QuinnAmdError
    from quinn_amd.nns.mlp import MLP
    from quinn_amd.solvers import NN_Laplace
    torch.manual_seed(3)
    np.random.seed(3)
    rs = np.random.RandomState(3)
    x = rs.rand(200, 1) * 2 - 1
    y = np.sin(3 * x) + 0.05 * rs.randn(200, 1)
    net = MLP(1, 1, (128, 128), biasorno=True, activ='tanh').double()
    fit = dict(val=[x[:20], y[:20]], lrate=0.01, batch_size=50, nepochs=5, freq_out=1000)
    with pytest.raises(QuinnAmdError, match="16384"):
        NN_Laplace(net, la_type='ggn', nens=2, verbose=False).fit(x, y, **fit)
    la = NN_Laplace(net, la_type='kron', nens=2, verbose=False)
    p = la.nparams
    assert p == 16897
    # the peak restarts from what is LIVE: tensors of earlier tests that sit in uncollected reference cycles (6.5 GB after
    # the cfg3 full-size test) would count, and whether a collection has run since depends on which tests came in between
    import gc
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    la.fit(x, y, **fit)
    xg = np.linspace(-1, 1, 33)[:, None]
    ym, yv, _ = la.predict_glm(xg, msc=1)
    ye = la.predict_ens(xg, nens=8)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    print("kron p = 16897: peak device memory", peak, "bytes; a p x p matrix would be", 8 * p * p)
    assert peak < 8 * p * p
    assert ym.shape == (33, 1) and np.isfinite(ym).all() and np.isfinite(yv).all() and np.all(yv > 0)
    assert ye.shape == (8, 33, 1) and np.isfinite(ye).all()
    with pytest.raises(ValueError, match="16384"):
        la.dense_cov(0)


def test_kron_glm_agrees_with_sampled_predictive_for_a_tight_posterior():
    """The design of test_glm_agrees_with_sampled_predictive_for_a_tight_posterior (test_gpu_glm.py) with la_type='kron':
    with cov_scale = 1e8 the network is linear across the posterior, so the variance of M = 4000 draws of qn_kron_sample agrees
    with qn_mlp_kron_glm_predict within 5 sqrt(2 / (M - 1)) relative."""
    from quinn_amd.nns.mlp import MLP
    from quinn_amd.solvers import NN_Laplace
    torch.manual_seed(1)
    np.random.seed(1)
    xtrn, ytrn, xval, yval = _ufit_data()
    net = MLP(1, 1, (8, 8), biasorno=True, activ='tanh').double()
    la = NN_Laplace(net, la_type='kron', nens=1, dfrac=1.0, cov_scale=STAT["cov_scale"], verbose=False)
    la.fit(xtrn, ytrn, val=[xval, yval], lrate=0.01, batch_size=4, nepochs=100, freq_out=1000)
    xg = np.linspace(-np.pi, np.pi, 9)[:, None]
    M = STAT["M"]
    np.random.seed(2)
    ms, vs, _ = la.predict_mom_sample(xg, msc=1, nsam=M)
    mg, vg, _ = la.predict_glm(xg, msc=1)
    rel = np.abs(vs - vg) / vg
    print("kron sampled vs glm variance, relative:", rel.ravel(), "margin", 5 * np.sqrt(2 / (M - 1)))
    assert np.all(rel <= 5 * np.sqrt(2 / (M - 1)))


def test_ex_ufit_laplace_kron_runs():
    import importlib.util
    path = os.path.join(HERE, "..", "examples", "ex_ufit.py")
    spec = importlib.util.spec_from_file_location("ex_ufit_laplace_kron", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    np.random.seed(0)
    torch.manual_seed(0)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        ymean, ystd, rmse = mod.main('laplace_kron', quick=True, mlp=True)
    assert ymean.shape == (11,) and ystd.shape == (11,) and np.isfinite(ymean).all()
