"""CPU: the Gauss-Newton curvature (csrc/qn_curv.hip, GGN kinds) and the linearised predictive (csrc/qn_glm.hip) restated in
numpy against torch.func Jacobians, the workspace queries / refusals of the new entry points (no device needed), the
argument checks and the mixture combine of NN_Laplace.predict_glm."""
import ctypes

import numpy as np
import pytest
import torch

from quinn_amd import _lib
from quinn_amd.ops import MLPArch, RNetArch, check_curvature_args


def _layers(arch, w):
    Ws, bs, off = [], [], 0
    for a, b in zip(arch.dims[:-1], arch.dims[1:]):
        Ws.append(w[off:off + a * b].reshape(b, a))
        off += a * b
        if arch.bias:
            bs.append(w[off:off + b])
            off += b
        else:
            bs.append(np.zeros(b))
    return Ws, bs


def jac_rows_np(arch, w, x):
    """(f [N, o], ins, gk) by the kernel's recurrences (k_jac_rows): ins[i] = ~in_i [e_i, N]; gk[k][i] = g^k_i [h_{i+1}, N], the
    backward pass started from the output unit vector e_k."""
    Ws, bs = _layers(arch, w)
    L, N, o = len(Ws), x.shape[0], arch.dims[-1]
    tl = lambda v: np.concatenate([v, np.ones((1, N))]) if arch.bias else v     # noqa: E731
    ins, sp = [x.T], []
    for i in range(L):
        z = Ws[i] @ ins[-1] + bs[i][:, None]
        if i + 1 < L:
            if arch.activ == "tanh":
                a = np.tanh(z); d1 = 1 - a * a
            elif arch.activ == "relu":
                a = np.maximum(z, 0); d1 = (a > 0).astype(float)
            else:
                a = z; d1 = np.ones_like(z)
            ins.append(a); sp.append(d1)
        else:
            f = z
    gk = []
    for k in range(o):
        g = [None] * L
        g[L - 1] = np.zeros((o, N)); g[L - 1][k] = 1.0
        for i in range(L - 2, -1, -1):
            g[i] = sp[i] * (Ws[i + 1].T @ g[i + 1])
        gk.append(g)
    return f.T, [tl(v) for v in ins], gk


def jac_np(arch, w, x):
    """J [N, o, p] assembled per layer block: J_nk[(i, a, b)] = g^k_i[a] ~in_i[b] (weights row-major, then the biases)."""
    f, ins, gk = jac_rows_np(arch, w, x)
    N, o = x.shape[0], arch.dims[-1]
    J = np.zeros((N, o, arch.nparams))
    for k in range(o):
        off = 0
        for i, (di, do) in enumerate(zip(arch.dims[:-1], arch.dims[1:])):
            blk = gk[k][i][:, None, :] * ins[i][None, :, :]                   # [do, e_i, N]
            J[:, k, off:off + di * do] = blk[:, :di, :].reshape(di * do, N).T
            off += di * do
            if arch.bias:
                J[:, k, off:off + do] = blk[:, di, :].T
                off += do
    return f, J


def ggn_np(arch, w, x):
    """(G [p, p], its diagonal) as the kernels form them: the sum over the outputs folded into one factor per row."""
    _, J = jac_np(arch, w, x)
    Jf = J.reshape(-1, arch.nparams)
    return Jf.T @ Jf, (Jf ** 2).sum(0)


def glm_np(arch, w, x, Sigma):
    f, J = jac_np(arch, w, x)
    T = J @ Sigma if Sigma.ndim == 2 else J * Sigma
    return f, np.einsum("nkp,nlp->nkl", T, J)


def torch_net(arch):
    act = {"tanh": torch.tanh, "relu": torch.relu, "identity": lambda v: v}[arch.activ]

    def f(w, xn):
        h, off = xn, 0
        L = len(arch.dims) - 1
        for i, (a, b) in enumerate(zip(arch.dims[:-1], arch.dims[1:])):
            h = w[off:off + a * b].view(b, a) @ h
            off += a * b
            if arch.bias:
                h = h + w[off:off + b]
                off += b
            if i + 1 < L:
                h = act(h)
        return h
    return f


def jac_autograd(arch, w, x):
    """J [N, o, p] by torch.func (float64)."""
    f = torch_net(arch)
    return torch.func.vmap(torch.func.jacrev(f), in_dims=(None, 0))(torch.as_tensor(w), torch.as_tensor(x)).numpy()


CASES = [((1, 6, 5, 1), "tanh", True), ((3, 7, 2), "relu", True), ((2, 5, 9, 4), "tanh", False),
         ((4, 6, 2), "identity", True), ((2, 3, 8, 5, 4), "tanh", True), ((3, 10, 1), "relu", False),
         ((2, 4, 4), "identity", False)]


@pytest.mark.parametrize("dims,act,bias", CASES)
def test_recurrences_match_autograd(dims, act, bias):
    arch = MLPArch(dims, act, bias)
    rs = np.random.RandomState(len(dims) * 100 + dims[-1])
    x = rs.randn(23, dims[0])
    w = rs.randn(arch.nparams) / np.sqrt(max(dims))
    p = arch.nparams
    Jr = jac_autograd(arch, w, x)
    G, Gd = ggn_np(arch, w, x)
    ref = np.einsum("nkp,nkq->pq", Jr, Jr)
    assert np.max(np.abs(G - ref)) <= 1e-12 * np.max(np.abs(ref))
    assert np.max(np.abs(Gd - np.diag(ref))) <= 1e-12 * np.max(np.abs(ref))
    A = rs.randn(p, p)
    Sigma = A @ A.T / p + 0.5 * np.eye(p)
    for Sg in (Sigma, 0.1 + rs.rand(p)):
        f, S = glm_np(arch, w, x, Sg)
        Sref = np.einsum("nkp,pq,nlq->nkl", Jr, Sg if Sg.ndim == 2 else np.diag(Sg), Jr)
        assert np.max(np.abs(S - Sref)) <= 1e-12 * np.max(np.abs(Sref))
        fref = torch.func.vmap(torch_net(arch), in_dims=(None, 0))(torch.as_tensor(w), torch.as_tensor(x)).numpy()
        assert np.max(np.abs(f - fref)) <= 1e-12 * np.max(np.abs(fref))


@pytest.fixture(scope="module")
def L():
    _lib.build()
    return _lib.lib()


def _desc(L, dims, act=1, bias=1):
    arr = (ctypes.c_int * len(dims))(*dims)
    h = ctypes.c_void_p()
    assert L.qn_mlp_desc_create(arr, len(dims), act, bias, ctypes.byref(h)) == 0
    return h


def test_ggn_workspace_without_device(L):
    h = _desc(L, (1, 64, 64, 64, 1))
    assert L.qn_curv_workspace_bytes(h, _lib.CURV_GGN_FULL, 8, 4096) > 0
    assert L.qn_curv_workspace_bytes(h, _lib.CURV_GGN_DIAG, 8, 4096) > 0
    assert (_lib.CURV_GGN_FULL, _lib.CURV_GGN_DIAG) == (2, 3)
    assert L.qn_curv_workspace_bytes(h, 7, 8, 4096) == 0
    L.qn_mlp_desc_destroy(h)
    big = _desc(L, (1, 128, 128, 1))                        # p = 16 897 > 16 384
    assert L.qn_curv_workspace_bytes(big, _lib.CURV_GGN_FULL, 1, 100) == 0
    assert b"16384" in L.qn_last_error()
    assert L.qn_curv_workspace_bytes(big, _lib.CURV_GGN_DIAG, 1, 100) > 0
    assert L.qn_mlp_curv(big, _lib.CURV_GGN_FULL, None, None, None, None, 1, 100, 100, None, None, 0, None) == -1
    L.qn_mlp_desc_destroy(big)


def _rnet(L):
    coef = (ctypes.c_double * 2)(1.0, 1.0)
    h = ctypes.c_void_p()
    assert L.qn_rnet_desc_create(1, 3, 1, 2, 1, coef, 1, 1, 1, 1, 0, ctypes.byref(h)) == 0
    return h


def test_glm_workspace_without_device(L):
    h = _desc(L, (1, 64, 64, 64, 1))
    p, o = 8513, 1
    assert L.qn_glm_workspace_bytes(h, _lib.GLM_COV_FULL, 8, 4096) > 0
    assert L.qn_glm_workspace_bytes(h, _lib.GLM_COV_DIAG, 8, 4096) > 0
    N = 16384
    ws = L.qn_glm_workspace_bytes(h, _lib.GLM_COV_FULL, 1, N)
    assert 0 < ws < 8 * N * o * p                          # the Jacobian [N, o, p] is not materialised
    assert L.qn_glm_workspace_bytes(h, 5, 1, 100) == 0
    assert b"cov_kind" in L.qn_last_error()
    assert L.qn_mlp_glm_predict(h, 5, None, None, None, 1, 100, None, None, None, 0, None) == -1
    L.qn_mlp_desc_destroy(h)
    big = _desc(L, (1, 128, 128, 1))
    assert L.qn_glm_workspace_bytes(big, _lib.GLM_COV_FULL, 1, 100) == 0
    assert b"16384" in L.qn_last_error()
    assert L.qn_glm_workspace_bytes(big, _lib.GLM_COV_DIAG, 1, 100) > 0
    assert L.qn_mlp_glm_predict(big, _lib.GLM_COV_FULL, None, None, None, 1, 100, None, None, None, 0, None) == -1
    L.qn_mlp_desc_destroy(big)
    rn = _rnet(L)
    assert L.qn_glm_workspace_bytes(rn, _lib.GLM_COV_DIAG, 1, 10) == 0
    assert b"RNet" in L.qn_last_error()
    assert L.qn_mlp_glm_predict(rn, _lib.GLM_COV_DIAG, None, None, None, 1, 10, None, None, None, 0, None) == -1
    assert L.qn_curv_workspace_bytes(rn, _lib.CURV_GGN_DIAG, 1, 10) == 0
    assert b"RNet" in L.qn_last_error()
    L.qn_mlp_desc_destroy(rn)


def test_argument_checks():
    from quinn_amd.solvers import NN_Laplace
    arch = MLPArch((1, 8, 1))
    assert check_curvature_args(arch, "float64", "ggn") == _lib.CURV_GGN_FULL
    assert check_curvature_args(arch, "float64", "ggn_diag") == _lib.CURV_GGN_DIAG
    with pytest.raises(ValueError):
        check_curvature_args(arch, "float64", "kfac")
    with pytest.raises(ValueError, match="float64"):
        check_curvature_args(arch, "float32", "ggn")
    with pytest.raises(NotImplementedError, match="RNet"):
        check_curvature_args(RNetArch(1, 3, 1, 2, ((1.0,), (1.0,))), "float64", "ggn")
    net = torch.nn.Sequential(torch.nn.Linear(1, 4), torch.nn.Tanh(), torch.nn.Linear(4, 1)).double()
    assert NN_Laplace(net, la_type="ggn", nens=1)._kind() == "ggn"
    assert NN_Laplace(net, la_type="ggn_diag", nens=1)._kind() == "ggn_diag"
    with pytest.raises(NotImplementedError):
        NN_Laplace(net, la_type="kfac", nens=1)._kind()


def test_mixture_combine():
    from quinn_amd.solvers.nn_laplace import glm_mixture
    rs = np.random.RandomState(4)
    N, o = 5, 2
    f = rs.randn(1, N, o)
    A = rs.randn(1, N, o, o)
    S = A @ np.swapaxes(A, -1, -2)
    m, c = glm_mixture(f, S)                                   # M = 1: the member itself
    assert np.array_equal(m, f[0]) and np.max(np.abs(c - S[0])) <= 1e-14 * (np.max(np.abs(S)) + np.max(f ** 2))
    f = rs.randn(2, N, o)
    A = rs.randn(2, N, o, o)
    S = A @ np.swapaxes(A, -1, -2)
    m, c = glm_mixture(f, S)
    for n in range(N):                                         # law of total variance, written out
        mu = 0.5 * (f[0, n] + f[1, n])
        within = 0.5 * (S[0, n] + S[1, n])
        between = 0.5 * (np.outer(f[0, n] - mu, f[0, n] - mu) + np.outer(f[1, n] - mu, f[1, n] - mu))
        assert np.allclose(m[n], mu, rtol=0, atol=1e-14)
        assert np.allclose(c[n], within + between, rtol=0, atol=1e-13)
    dn = 0.3
    m2, c2 = glm_mixture(f, S, dn ** 2)
    assert np.array_equal(m2, m)
    assert np.allclose(c2 - c, dn ** 2 * np.eye(o)[None], rtol=0, atol=1e-14)
