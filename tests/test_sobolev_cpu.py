"""CPU: the input Jacobian and the derivative-informed loss (csrc/qn_sobolev.hip) -- the reverse recursion of the kernels
restated in numpy against torch float64 autograd, the exported symbols, the workspace query / refusals (no device needed) and
the argument checks of GradLoss and loss_fn='gradloss'."""
import ctypes

import numpy as np
import pytest
import torch

from quinn_amd import _lib
from quinn_amd.ops import MLPArch, RNetArch, check_sobolev_args, check_gradloss_args


# ---------------------------------------------------------------- the yardstick: torch float64 autograd on the CPU
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


def jac_x_autograd(arch, w, x):
    """(f [N, o], J [N, o, d]) as torch tensors (differentiable in w when w requires grad)."""
    f = torch_net(arch)
    w, x = torch.as_tensor(w), torch.as_tensor(x)
    pred = torch.func.vmap(f, in_dims=(None, 0))(w, x)
    J = torch.func.vmap(torch.func.jacrev(f, argnums=1), in_dims=(None, 0))(w, x)
    return pred, J


def sobolev_autograd(arch, w, x, y, g, wv, wg):
    """(sse, gsse, d (wv sse + wg gsse) / dw) by torch.autograd.grad of the scalar loss."""
    wt = torch.tensor(np.asarray(w, dtype=np.float64), requires_grad=True)
    pred, J = jac_x_autograd(arch, wt, x)
    sse = ((pred - torch.as_tensor(y)) ** 2).sum()
    gsse = ((J - torch.as_tensor(g)) ** 2).sum()
    grad, = torch.autograd.grad(wv * sse + wg * gsse, wt)
    return sse.item(), gsse.item(), grad.numpy()


# ---------------------------------------------------------------- the kernels' recursion in numpy
def _layers(arch, w):
    Ws, bs, off = [], [], 0
    for a, b in zip(arch.dims[:-1], arch.dims[1:]):
        Ws.append(w[off:off + a * b].reshape(b, a))
        off += a * b
        bs.append(w[off:off + b] if arch.bias else np.zeros(b))
        off += b if arch.bias else 0
    return Ws, bs


def sobolev_np(arch, w, x, y, g, wv, wg):
    """(f [N, o], J [N, o, d], sse, gsse, grad [p]) by the tangent forward and the reverse pass over it, as the kernels run
    them: per layer a [h, N] and the tangents da [d, h, N]; zb / dzb the adjoints of z and dz^j."""
    Ws, bs = _layers(arch, w)
    L, (N, d) = len(Ws), x.shape
    a, da = [x.T], [np.broadcast_to(np.eye(d)[:, :, None], (d, d, N)).copy()]
    for l in range(L):
        z = Ws[l] @ a[l] + bs[l][:, None]
        dz = np.einsum("ck,jkn->jcn", Ws[l], da[l])
        if l + 1 < L:
            if arch.activ == "tanh":
                al = np.tanh(z); d1 = 1 - al * al
            elif arch.activ == "relu":
                al = np.maximum(z, 0); d1 = (al > 0).astype(float)
            else:
                al = z; d1 = np.ones_like(z)
            a.append(al); da.append(d1 * dz)
    f, J = z.T, dz.transpose(2, 1, 0)                                   # [N, o], [N, o, d]
    sse, gsse = np.sum((f - y) ** 2), np.sum((J - g) ** 2)
    zb = 2 * wv * (f - y).T                                             # [o, N]
    dzb = 2 * wg * (J - g).transpose(2, 1, 0)                           # [d, o, N]
    grads = [None] * L
    for l in range(L - 1, -1, -1):
        gW = zb @ a[l].T + np.einsum("jcn,jkn->ck", dzb, da[l])
        grads[l] = (gW, zb.sum(1))
        if l == 0:
            break
        ab = Ws[l].T @ zb
        dab = np.einsum("ck,jcn->jkn", Ws[l], dzb)
        al = a[l]
        if arch.activ == "tanh":
            d1 = 1 - al * al
            zb = d1 * ab + np.sum(-2 * al * da[l] * dab, axis=0)       # act''(z) dz^j = -2 a da^j
        elif arch.activ == "relu":
            d1 = (al > 0).astype(float)
            zb = d1 * ab
        else:
            d1 = np.ones_like(al)
            zb = ab
        dzb = d1 * dab
    flat = []
    for gW, gb in grads:
        flat.append(gW.ravel())
        if arch.bias:
            flat.append(gb)
    return f, J, sse, gsse, np.concatenate(flat)


CASES = [((1, 6, 5, 1), "tanh", True), ((3, 7, 2), "relu", True), ((2, 5, 9, 4), "tanh", False),
         ((4, 6, 2), "identity", True), ((2, 3, 8, 5, 4), "tanh", True), ((3, 10, 1), "relu", False),
         ((2, 4, 4), "identity", False), ((16, 9, 3), "tanh", True)]


@pytest.mark.parametrize("dims,act,bias", CASES)
def test_recursion_matches_autograd(dims, act, bias):
    arch = MLPArch(dims, act, bias)
    rs = np.random.RandomState(len(dims) * 100 + dims[0])
    N, d, o = 23, dims[0], dims[-1]
    x, y, g = rs.randn(N, d), rs.randn(N, o), rs.randn(N, o, d)
    w = rs.randn(arch.nparams) / np.sqrt(max(dims))
    pref, Jref = jac_x_autograd(arch, w, x)
    for wv, wg in ((1.0, 0.0), (0.0, 1.0), (1.0, 0.37)):
        f, J, sse, gsse, grad = sobolev_np(arch, w, x, y, g, wv, wg)
        sref, gref, dref = sobolev_autograd(arch, w, x, y, g, wv, wg)
        assert np.max(np.abs(f - pref.numpy())) <= 1e-12 * np.max(np.abs(pref.numpy()))
        assert np.max(np.abs(J - Jref.numpy())) <= 1e-12 * np.max(np.abs(Jref.numpy()))
        assert abs(sse - sref) <= 1e-12 * sref and abs(gsse - gref) <= 1e-12 * gref
        assert np.max(np.abs(grad - dref)) <= 1e-11 * np.max(np.abs(dref))


# ---------------------------------------------------------------- C ABI without a device
@pytest.fixture(scope="module")
def L():
    _lib.build()
    return _lib.lib()


def _desc(L, dims, act=1, bias=1):
    arr = (ctypes.c_int * len(dims))(*dims)
    h = ctypes.c_void_p()
    assert L.qn_mlp_desc_create(arr, len(dims), act, bias, ctypes.byref(h)) == 0
    return h


def _rnet(L):
    coef = (ctypes.c_double * 2)(1.0, 1.0)
    h = ctypes.c_void_p()
    assert L.qn_rnet_desc_create(1, 3, 1, 2, 1, coef, 1, 1, 1, 1, 0, ctypes.byref(h)) == 0
    return h


def test_symbols_exported(L):
    for name in ("qn_sobolev_workspace_bytes", "qn_mlp_input_jac", "qn_mlp_sobolev_fwdbwd"):
        assert name in _lib.SYMBOLS
        assert hasattr(L, name)
    assert "qn_sobolev.hip" in _lib.SOURCES


def test_workspace_without_device(L):
    h = _desc(L, (6, 64, 64, 64, 1))
    p = 6 * 64 + 64 + 2 * (64 * 64 + 64) + 64 + 1
    fwd = L.qn_sobolev_workspace_bytes(h, 8, 4096, 0)
    bwd = L.qn_sobolev_workspace_bytes(h, 8, 4096, 1)
    assert 0 < fwd < bwd
    # rows go in tiles: the workspace stops growing with N, and never holds N x p
    big = L.qn_sobolev_workspace_bytes(h, 1, 1 << 20, 1)
    assert 0 < big < 8 * (1 << 20) * p // 64
    assert big < 2 * L.qn_sobolev_workspace_bytes(h, 1, 1 << 14, 1)
    assert L.qn_sobolev_workspace_bytes(h, 0, 100, 1) == 0
    assert L.qn_sobolev_workspace_bytes(h, 1, 0, 1) == 0
    L.qn_mlp_desc_destroy(h)


@pytest.mark.parametrize("dims,what", [((17, 8, 1), b"d = 17"), ((2, 8, 17), b"o = 17")])
def test_wide_input_output_refused(L, dims, what):
    h = _desc(L, dims)
    assert L.qn_sobolev_workspace_bytes(h, 1, 10, 1) == 0
    assert what in L.qn_last_error()
    assert L.qn_mlp_input_jac(h, None, None, None, 1, 10, 10, None, None, None, 0, None) == -1
    assert what in L.qn_last_error()
    assert L.qn_mlp_sobolev_fwdbwd(h, None, None, None, None, None, 1, 10, 10, 1.0, 1.0, None, None, None, None, 0, None) == -1
    L.qn_mlp_desc_destroy(h)


def test_rnet_refused(L):
    rn = _rnet(L)
    assert L.qn_sobolev_workspace_bytes(rn, 1, 10, 0) == 0
    assert b"RNet" in L.qn_last_error()
    assert L.qn_mlp_input_jac(rn, None, None, None, 1, 10, 10, None, None, None, 0, None) == -1
    assert L.qn_mlp_sobolev_fwdbwd(rn, None, None, None, None, None, 1, 10, 10, 1.0, 1.0, None, None, None, None, 0, None) == -1
    assert b"RNet" in L.qn_last_error()
    L.qn_mlp_desc_destroy(rn)


def test_null_arguments_refused(L):
    h = _desc(L, (2, 8, 1))
    assert L.qn_mlp_input_jac(h, None, None, None, 1, 10, 10, None, None, None, 0, None) == -1
    assert L.qn_mlp_sobolev_fwdbwd(h, None, None, None, None, None, 1, 10, 10, 1.0, 1.0, None, None, None, None, 0, None) == -1
    L.qn_mlp_desc_destroy(h)


# ---------------------------------------------------------------- Python argument checks
def test_check_sobolev_args():
    arch = MLPArch((2, 8, 1))
    check_sobolev_args(arch, "float64")
    with pytest.raises(ValueError, match="float64"):
        check_sobolev_args(arch, "float32")
    with pytest.raises(NotImplementedError, match="d <= 16"):
        check_sobolev_args(MLPArch((17, 8, 1)), "float64")
    with pytest.raises(NotImplementedError, match="o <= 16"):
        check_sobolev_args(MLPArch((2, 8, 17)), "float64")
    rn = RNetArch(1, 3, 1, 2, ((1.0,), (1.0,)), layer_pre=True, layer_post=True)
    with pytest.raises(NotImplementedError, match="RNet"):
        check_sobolev_args(rn, "float64")


def test_check_gradloss_args_shapes():
    x = np.zeros((5, 2))
    a1, a3 = MLPArch((2, 8, 1)), MLPArch((2, 8, 3))
    assert check_gradloss_args(a1, "float64", x, np.ones((5, 2)), 0.5).shape == (5, 1, 2)
    assert check_gradloss_args(a1, "float64", x, torch.ones(5, 1, 2), 0.0).shape == (5, 1, 2)
    assert check_gradloss_args(a3, "float64", x, np.ones((5, 3, 2)), 1.0).shape == (5, 3, 2)
    for bad in (np.ones((5, 2)), np.ones((4, 3, 2)), np.ones((5, 2, 3))):
        with pytest.raises(ValueError, match="gtrn has shape"):
            check_gradloss_args(a3, "float64", x, bad, 1.0)
    with pytest.raises(ValueError, match="needs gtrn"):
        check_gradloss_args(a1, "float64", x, None, 1.0)
    for lam in (-1.0, float("nan"), None):
        with pytest.raises(ValueError, match="lam"):
            check_gradloss_args(a1, "float64", x, np.ones((5, 2)), lam)


def _mlp(d=2, o=1):
    return torch.nn.Sequential(torch.nn.Linear(d, 6), torch.nn.Tanh(), torch.nn.Linear(6, o)).double()


def test_gradloss_argument_checks():
    from quinn_amd.nns.losses import GradLoss
    net, x = _mlp(), np.zeros((5, 2))
    loss = GradLoss(net, lam=0.3, xtrn=x, gtrn=np.ones((5, 2)))
    assert loss.lam == 0.3 and loss.xtrn.shape == (5, 2) and loss.gtrn.shape == (5, 1, 2)
    with pytest.raises(ValueError, match="xtrn"):
        GradLoss(net, lam=0.3, gtrn=np.ones((5, 2)))
    with pytest.raises(ValueError, match="needs gtrn"):
        GradLoss(net, lam=0.3, xtrn=x)
    with pytest.raises(ValueError, match="gtrn has shape"):
        GradLoss(net, lam=0.3, xtrn=x, gtrn=np.ones((4, 2)))
    with pytest.raises(ValueError, match="lam"):
        GradLoss(net, lam=-0.3, xtrn=x, gtrn=np.ones((5, 2)))
    with pytest.raises(ValueError, match="float64"):
        GradLoss(net, lam=0.3, xtrn=x, gtrn=np.ones((5, 2)), dtype="float32")
    assert "attribute" in GradLoss.__doc__ or "_xtrn" in GradLoss.__doc__


def test_nnfit_gradloss_argument_checks():
    """Everything is refused before a device is needed."""
    from quinn_amd.nns.nnfit import nnfit
    net, x, y = _mlp(), np.zeros((5, 2)), np.zeros((5, 1))
    for lp in (None, {}, {'lam': 1.0}):
        with pytest.raises(ValueError, match="lossparams"):
            nnfit(net, x, y, loss_fn='gradloss', lossparams=lp, nepochs=1)
    with pytest.raises(ValueError, match="gtrn has shape"):
        nnfit(net, x, y, loss_fn='gradloss', lossparams={'gtrn': np.ones((5, 3)), 'lam': 1.0}, nepochs=1)
    with pytest.raises(ValueError, match="lam"):
        nnfit(net, x, y, loss_fn='gradloss', lossparams={'gtrn': np.ones((5, 2)), 'lam': -1.0}, nepochs=1)
    with pytest.raises(ValueError, match="float64"):
        nnfit(net, x, y, loss_fn='gradloss', lossparams={'gtrn': np.ones((5, 2)), 'lam': 1.0}, nepochs=1, dtype="float32")


def test_mcmc_gradient_data_argument_checks():
    from quinn_amd.solvers.nn_mcmc import NN_MCMC
    s = NN_MCMC(_mlp(), verbose=False)
    x, y, g = np.zeros((5, 2)), np.zeros((5, 1)), np.ones((5, 2))
    with pytest.raises(NotImplementedError, match="engine='host'"):
        s.fit(x, y, gtrn=g, gradnoise=0.1, engine='device', sampler_params={})
    with pytest.raises(ValueError, match="gradnoise"):
        s.fit(x, y, gtrn=g, sampler_params={})
    with pytest.raises(ValueError, match="gradnoise"):
        s.fit(x, y, gradnoise=0.1, sampler_params={})
    with pytest.raises(ValueError, match="gtrn has shape"):
        s.fit(x, y, gtrn=np.ones((5, 3)), gradnoise=0.1, sampler_params={})
