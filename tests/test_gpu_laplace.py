"""GPU: the curvature kernels (qn_mlp_curv, csrc/qn_curv.hip) against torch autograd and the reference's recorded
Hessians, and NN_Laplace end to end against the reference's recorded run (tests/golden/g14_*.npz)."""
import os

import numpy as np
import pytest
import torch

from quinn_amd.ops import MLPArch, BatchedMLP

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _torch_loss(arch, x, y):
    """w -> sum_n |f_w(x_n) - y_n|^2 / 2 in torch float64 (CPU)."""
    X = torch.as_tensor(x, dtype=torch.float64)
    Y = torch.as_tensor(y, dtype=torch.float64)
    act = {"tanh": torch.tanh, "relu": torch.relu, "identity": lambda v: v}[arch.activ]

    def f(w):
        h, off = X, 0
        L = len(arch.dims) - 1
        for i, (a, b) in enumerate(zip(arch.dims[:-1], arch.dims[1:])):
            Wl = w[off:off + a * b].view(b, a)
            off += a * b
            h = h @ Wl.T
            if arch.bias:
                h = h + w[off:off + b]
                off += b
            if i + 1 < L:
                h = act(h)
        return 0.5 * ((h - Y) ** 2).sum()
    return f


def _hess_ref(arch, w, x, y):
    return torch.autograd.functional.hessian(_torch_loss(arch, x, y), torch.as_tensor(w, dtype=torch.float64)).numpy()


def _diag_ref(arch, w, x, y):
    g = []
    for n in range(x.shape[0]):
        wt = torch.as_tensor(w, dtype=torch.float64).clone().requires_grad_(True)
        l = _torch_loss(arch, x[n:n + 1], y[n:n + 1])(wt)
        g.append(torch.autograd.grad(l, wt)[0].numpy())
    return np.mean(np.square(np.array(g)), axis=0)


ARCHS = [((1, 16, 16, 1), "tanh", True), ((3, 7, 2), "relu", True), ((2, 5, 70, 3), "tanh", False),
         ((16, 33, 4), "identity", True), ((4, 1, 9, 17, 8, 2), "tanh", True), ((5, 64, 64, 1), "relu", False)]


@pytest.mark.parametrize("dims,act,bias", ARCHS)
@pytest.mark.parametrize("N", [1, 63, 1000])
def test_full_hessian_vs_autograd(dims, act, bias, N):
    arch = MLPArch(dims, act, bias)
    rs = np.random.RandomState(hash((dims, act, bias, N)) % 2 ** 31)
    x = rs.randn(N, dims[0])
    y = rs.randn(N, dims[-1])
    B = 3
    W = rs.randn(B, arch.nparams) / np.sqrt(max(dims))
    nb = max(1, (2 * N) // 3)
    rows = np.stack([rs.permutation(N)[:nb] for _ in range(B)]).astype(np.int32)
    op = BatchedMLP(arch, x, y, device="cuda:0")
    H = op.curvature(W, "full", row_idx=rows).cpu().numpy()
    for b in range(B):
        ref = _hess_ref(arch, W[b], x[rows[b]], y[rows[b]])
        assert np.array_equal(H[b], H[b].T)
        assert np.max(np.abs(H[b] - ref)) <= 1e-11 * np.max(np.abs(ref)), (b, np.max(np.abs(H[b] - ref)), np.max(np.abs(ref)))


@pytest.mark.parametrize("dims,act,bias", ARCHS[:4])
def test_diag_vs_per_row_gradients(dims, act, bias):
    arch = MLPArch(dims, act, bias)
    rs = np.random.RandomState(7)
    x = rs.randn(150, dims[0])
    y = rs.randn(150, dims[-1])
    W = rs.randn(2, arch.nparams) / np.sqrt(max(dims))
    op = BatchedMLP(arch, x, y, device="cuda:0")
    D = op.curvature(W, "diag").cpu().numpy()
    for b in range(2):
        ref = _diag_ref(arch, W[b], x, y)
        assert np.max(np.abs(D[b] - ref)) <= 1e-12 * np.max(np.abs(ref))


def test_diag_cfg2_size():
    """DIAG of 8 members of the 3x64 network on 4096 rows against a float64 per-row-gradient computation (vmapped autograd)."""
    arch = MLPArch((1, 64, 64, 64, 1), "tanh")
    rs = np.random.RandomState(3)
    N = 4096
    x = rs.rand(N, 1) * 2 - 1
    y = np.sin(3 * x) + 0.1 * rs.randn(N, 1)
    W = rs.randn(8, arch.nparams) / 8
    op = BatchedMLP(arch, x, y, device="cuda:0")
    D = op.curvature(W, "diag").cpu().numpy()
    for b in (0, 5):
        f = lambda w, xn, yn: _torch_loss(arch, xn[None], yn[None])(w)   # noqa: E731
        wt = torch.as_tensor(W[b])
        g = torch.func.vmap(torch.func.grad(lambda w, xn, yn: _per_row(arch, w, xn, yn)), in_dims=(None, 0, 0))(
            wt, torch.as_tensor(x), torch.as_tensor(y))
        ref = (g ** 2).mean(0).numpy()
        assert np.max(np.abs(D[b] - ref)) <= 1e-12 * np.max(np.abs(ref))


def _per_row(arch, w, xn, yn):
    h, off = xn, 0
    L = len(arch.dims) - 1
    for i, (a, b) in enumerate(zip(arch.dims[:-1], arch.dims[1:])):
        h = w[off:off + a * b].view(b, a) @ h
        off += a * b
        if arch.bias:
            h = h + w[off:off + b]
            off += b
        if i + 1 < L:
            h = torch.tanh(h) if arch.activ == "tanh" else torch.relu(h) if arch.activ == "relu" else h
    return 0.5 * ((h - yn) ** 2).sum()


def test_curvature_deterministic():
    arch = MLPArch((2, 40, 40, 1), "tanh")
    rs = np.random.RandomState(11)
    x, y = rs.randn(700, 2), rs.randn(700, 1)
    W = rs.randn(2, arch.nparams) / 6
    op = BatchedMLP(arch, x, y, device="cuda:0")
    for kind in ("full", "diag"):
        a = op.curvature(W, kind).cpu().numpy()
        b = op.curvature(W, kind).cpu().numpy()
        assert np.array_equal(a, b), kind


def test_full_hessian_over_several_row_tiles():
    """Nb above one row tile (the tangent workspace bounds it at 1024 / fewer rows for wide nets): the sum of the
    Hessians of two row subsets, each one tile, equals the Hessian of all rows."""
    arch = MLPArch((3, 100, 100, 2), "tanh")
    rs = np.random.RandomState(21)
    x, y = rs.randn(1500, 3), rs.randn(1500, 2)
    W = rs.randn(1, arch.nparams) / 10
    op = BatchedMLP(arch, x, y, device="cuda:0")
    H = op.curvature(W, "full")[0]
    r = np.arange(1500, dtype=np.int32)
    H1 = op.curvature(W, "full", row_idx=r[None, :700])[0]
    H2 = op.curvature(W, "full", row_idx=r[None, 700:])[0]
    scale = torch.max(torch.abs(H)).item()
    assert torch.max(torch.abs(H - H1 - H2)).item() <= 1e-12 * scale
    assert torch.equal(H, H.T)


def test_diag_over_several_row_tiles():
    arch = MLPArch((2, 9, 3), "relu")
    rs = np.random.RandomState(22)
    x, y = rs.randn(9000, 2), rs.randn(9000, 3)
    W = rs.randn(1, arch.nparams) / 3
    op = BatchedMLP(arch, x, y, device="cuda:0")
    D = op.curvature(W, "diag").cpu().numpy()[0]
    g = torch.func.vmap(torch.func.grad(lambda w, xn, yn: _per_row(arch, w, xn, yn)), in_dims=(None, 0, 0))(
        torch.as_tensor(W[0]), torch.as_tensor(x), torch.as_tensor(y))
    ref = (g ** 2).mean(0).numpy()
    assert np.max(np.abs(D - ref)) <= 1e-12 * np.max(np.abs(ref))


def _load(name):
    with np.load(os.path.join(GOLD, name), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def _mlp(g):
    from quinn_amd.nns.mlp import MLP
    dims = [int(v) for v in g["dims"]]
    bias = bool(g["bias"]) if "bias" in g else True
    return MLP(dims[0], dims[-1], tuple(dims[1:-1]), biasorno=bias, activ=str(g["activ"]))


@pytest.mark.parametrize("k", range(5))
def test_nnwrap_hessians_vs_reference(k):
    from quinn_amd.nns.nnwrap import NNWrap
    from quinn_amd.nns.losses import NegLogPost
    g = _load(f"g14_hess_{k}.npz")
    net = _mlp(g)
    nw = NNWrap(net)
    loss = NegLogPost(net, g["x"].shape[0], float(g["sigma"]), None)
    H = nw.calc_hess_full(g["w"], loss, g["x"], g["y"])
    ref = g["hess_full"]
    assert H.shape == ref.shape and np.array_equal(H, H.T)
    assert np.max(np.abs(H - ref)) <= 1e-11 * np.max(np.abs(ref))
    Dm = nw.calc_hess_diag(g["w"], loss, g["x"], g["y"])
    assert Dm.shape == ref.shape and np.count_nonzero(Dm - np.diag(np.diag(Dm))) == 0
    refd = g["hess_diag"]
    assert np.max(np.abs(np.diag(Dm) - refd)) <= 1e-11 * np.max(np.abs(refd))
    with pytest.raises(NotImplementedError):
        nw.calc_hess_full(g["w"], NegLogPost(net, 5, 0.1, {"sigma": 1.0, "anchor": np.zeros(len(g["w"]))}), g["x"], g["y"])


@pytest.mark.parametrize("la_type", ["full", "diag"])
def test_nn_laplace_end_to_end_vs_reference(la_type):
    from quinn_amd.nns.nnfit import load_flat_into
    from quinn_amd.solvers import NN_Laplace
    g = _load(f"g14_laplace_{la_type}.npz")
    net = _mlp(g)
    load_flat_into(net, g["w0"])
    la = NN_Laplace(net, la_type=la_type, cov_scale=float(g["cov_scale"]), nens=int(g["nens"]), dfrac=float(g["dfrac"]),
                    verbose=False, datanoise=float(g["datanoise"]), priorsigma=float(g["priorsigma"]))
    np.random.seed(int(g["np_seed"]))
    torch.manual_seed(int(g["torch_seed"]))
    la.fit(g["x"], g["y"], val=[g["xval"], g["yval"]], lrate=float(g["lrate"]), batch_size=int(g["batch_size"]),
           nepochs=int(g["nepochs"]), freq_out=1000)
    assert np.array_equal(la.rows, g["rows"])
    np.testing.assert_allclose(np.array(la.means), g["means"], rtol=1e-9, atol=1e-11)     # G9's bars
    for H, ref in zip(la.hessians, g["hessians"]):
        assert np.max(np.abs(H - ref)) <= 1e-6 * np.max(np.abs(ref))       # weights differ by ~1e-9 after the MAP fit
    # prediction: the reference's draw sequence; with the fixture's means / covariances the draws match
    la.means = [m for m in g["means"]]
    la.cov_mats = [c for c in g["cov_mats"]]
    la._factors = [None] * len(la.means)
    np.random.seed(int(g["pred_seed"]))
    with pytest.warns(RuntimeWarning) if la_type == "full" else _nowarn():
        Wd = la._draw_weights(len(g["pred_jens"]))
    np.testing.assert_allclose(Wd, g["pred_thetas"], rtol=1e-9, atol=1e-9 * np.max(np.abs(g["pred_thetas"])))
    np.random.seed(int(g["pred_seed"]))
    jens = []
    for _ in range(len(g["pred_jens"])):                    # the reference's order: randint, then p standard normals
        jens.append(int(np.random.randint(0, la.nens)))
        np.random.standard_normal(la.nparams)
    assert jens == [int(v) for v in g["pred_jens"]]
    np.random.seed(int(g["pred_seed"]))
    y = la.predict_ens(g["xpred"], nens=len(g["pred_jens"]))
    np.testing.assert_allclose(y, g["pred"], rtol=1e-8, atol=1e-8 * np.max(np.abs(g["pred"])))
    np.random.seed(int(g["pred_seed"]))
    m, v, _ = la.predict_mom_sample(g["xpred"], msc=1, nsam=len(g["pred_jens"]))
    np.testing.assert_allclose(m, g["pred"].mean(0), rtol=1e-8, atol=1e-8 * np.max(np.abs(g["pred"])))
    # la_calc with batches: the sum of the per-batch results
    learner = la.learners[0]
    rows = g["rows"][0]
    H = la.la_calc(learner, g["x"][rows], g["y"][rows], batch_size=int(g["batch_k"])) if len(g["batch_cov"]) else \
        _batched_hess_only(la, learner, g["x"][rows], g["y"][rows], int(g["batch_k"]))
    ref = g["batch_hessians"].sum(axis=0)
    assert np.max(np.abs(H - ref)) <= 1e-6 * np.max(np.abs(ref))


def _batched_hess_only(la, learner, x, y, k):
    try:
        return la.la_calc(learner, x, y, batch_size=k)
    except np.linalg.LinAlgError:                            # the reference's inverse failed there too
        import quinn_amd.solvers.nn_laplace as mod
        inv = np.linalg.inv
        got = {}
        mod.np.linalg.inv = lambda a: (got.setdefault("h", a), np.zeros_like(a))[1]
        try:
            la.la_calc(learner, x, y, batch_size=k)
        finally:
            mod.np.linalg.inv = inv
        return got["h"] / la.cov_scale


class _nowarn:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


def test_ex_ufit_laplace_runs():
    import importlib.util
    path = os.path.join(os.path.dirname(GOLD), "..", "examples", "ex_ufit.py")
    spec = importlib.util.spec_from_file_location("ex_ufit_laplace", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    np.random.seed(0)
    torch.manual_seed(0)
    ymean, ystd, rmse = mod.main('laplace', quick=True, mlp=True)
    assert ymean.shape == (11,) and ystd.shape == (11,) and np.isfinite(ymean).all()
