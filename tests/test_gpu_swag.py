"""GPU: the SWAG kernels (qn_swag_step / qn_swag_sample, csrc/qn_swag.hip) against numpy, bit for bit where the
arithmetic allows, and NN_SWAG end to end against the reference's recorded runs (tests/golden/g15_swag_*.npz)."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from conftest import load_golden
from quinn_amd import _lib
from quinn_amd.nns.mlp import MLP
from quinn_amd.nns.nnfit import load_flat_into
from quinn_amd.nns import rnet as R
from quinn_amd.ops import swag_sample, swag_step
from quinn_amd.solvers import NN_SWAG

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = "cuda:0"


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def _misaligned(a):
    """A contiguous device copy of `a` whose data start 8 bytes past a 16-byte boundary (the kernel's scalar path)."""
    buf = torch.empty(a.size + 1, dtype=torch.float64, device=DEV)
    t = buf[1:].view(a.shape)
    t.copy_(_dev(a))
    return t


def _step_np(W, G, lr, gscale, m1, m2, ring, n, slot):
    W = W - lr[:, None] * (G.astype(np.float64) * gscale)
    if n:
        m1 = (n * m1 + W) / (n + 1)
        m2 = (n * m2 + W * W) / (n + 1)
        if ring is not None:
            ring = ring.copy()
            ring[:, slot] = W - m1
    return W, m1, m2, ring


@pytest.mark.parametrize("B,p", [(1, 1), (1, 6), (7, 1001), (512, 333)])
@pytest.mark.parametrize("gdt", [np.float64, np.float32])
@pytest.mark.parametrize("aligned", [True, False])
def test_swag_step_bitwise(B, p, gdt, aligned):
    rs = np.random.RandomState(B * 7 + p)
    K, c, n_steps = 3, 2, 9                               # 4 collections: the ring wraps past K
    W = rs.randn(B, p)
    lr = rs.rand(B) * 0.1
    gscale = 1.0 / 37
    put = _dev if aligned else _misaligned
    Wd, m1d, m2d = put(W), put(np.zeros((B, p))), put(np.zeros((B, p)))
    Dd = put(np.zeros((B, K, p)))
    lrd = _dev(lr)
    swag_step(_lib.SWAG_INIT, Wd, m1=m1d, m2=m2d)
    m1, m2, ring = W.copy(), W * W, np.zeros((B, K, p))
    for i in range(1, n_steps + 1):
        G = (rs.randn(B, p) * 3).astype(gdt)
        n = i // c if i % c == 0 else 0
        Gd = _dev(G) if aligned or gdt == np.float32 else put(G)
        if n:
            swag_step(_lib.SWAG_SGD_COLLECT, Wd, Gd, lrd, gscale, m1d, m2d, Dd, slot=(n - 1) % K, n=n)
        else:
            swag_step(_lib.SWAG_SGD, Wd, Gd, lrd, gscale)
        W, m1, m2, ring = _step_np(W, G, lr, gscale, m1, m2, ring, n, (n - 1) % K)
    torch.cuda.synchronize()
    for name, got, ref in (("W", Wd, W), ("m1", m1d, m1), ("m2", m2d, m2), ("D", Dd, ring)):
        assert np.array_equal(got.cpu().numpy(), ref), name


def test_swag_step_constant_weights_negative_variance():
    """W does not move (G = 0): m2 - m1^2 is rounding noise, negative for about a quarter of the entries, as in numpy."""
    rs = np.random.RandomState(3)
    B, p = 2, 4096
    W = rs.randn(B, p)
    Wd, m1d, m2d = _dev(W), torch.empty(B, p, dtype=torch.float64, device=DEV), torch.empty(B, p, dtype=torch.float64, device=DEV)
    Gd, lrd = torch.zeros(B, p, dtype=torch.float64, device=DEV), _dev(np.full(B, 0.1))
    swag_step(_lib.SWAG_INIT, Wd, m1=m1d, m2=m2d)
    m1, m2 = W.copy(), W * W
    for n in range(1, 6):
        swag_step(_lib.SWAG_SGD_COLLECT, Wd, Gd, lrd, 1.0, m1d, m2d, None, n=n)
        m1 = (n * m1 + W) / (n + 1)
        m2 = (n * m2 + W * W) / (n + 1)
    diag = (m2d - m1d * m1d).cpu().numpy()
    assert np.array_equal(diag, m2 - m1 * m1)
    assert (diag < 0).any() and (diag > 0).any()
    assert np.array_equal(Wd.cpu().numpy(), W)


def _sample_np(means, diags, D, js, z1, z2, drift):
    """predict_sample's theta (nn_swag.py:125-145) in sequence; D [B, K, p] oldest row first, or None (diagonal)."""
    out = []
    for s, j in enumerate(js):
        with np.errstate(invalid="ignore"):
            corr = np.sqrt(diags[j]) * z1[s]
        if D is not None:
            K = D.shape[1]
            corr = np.sqrt(0.5) * corr + np.sqrt(0.5) * np.dot(D[j].T, z2[s]) / np.sqrt(K - 1)
        if drift:
            means[j] += corr
            out.append(means[j].copy())
        else:
            out.append(means[j] + corr)
    return np.array(out)


def _sample_inputs(B=5, K=4, p=777, M=40, seed=0):
    rs = np.random.RandomState(seed)
    means = rs.randn(B, p)
    diags = rs.rand(B, p) * 0.01
    diags[rs.rand(B, p) < 0.01] *= -1                    # negative variances: NaN, as np.sqrt gives
    D = rs.randn(B, K, p) * 0.1
    js = rs.randint(0, B, M)
    js[:6] = [1, 1, 3, 1, 3, 3]                          # repeated members within one call
    return means, diags, D, js, rs.randn(M, p), rs.randn(M, K)


def _close(got, ref, rtol):
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    ok = ~np.isnan(ref)
    scale = np.max(np.abs(ref[ok]))
    assert np.max(np.abs(got[ok] - ref[ok])) <= rtol * scale, np.max(np.abs(got[ok] - ref[ok])) / scale


@pytest.mark.parametrize("drift", [True, False])
def test_swag_sample_lowrank_vs_sequential_numpy(drift):
    means, diags, D, js, z1, z2 = _sample_inputs()
    md = _dev(means)
    th = swag_sample(md, _dev(diags), _dev(D), js, z1, z2, drift).cpu().numpy()
    mref = means.copy()
    ref = _sample_np(mref, diags, D, js, z1, z2, drift)
    _close(th, ref, 1e-14)                                # only D z2 is summed in an order of its own
    if drift:
        _close(md.cpu().numpy(), mref, 1e-14)
        assert np.isnan(md.cpu().numpy()).any()           # a NaN draw poisons its member's mean, as in the reference
    else:
        assert np.array_equal(md.cpu().numpy(), means)


@pytest.mark.parametrize("drift", [True, False])
def test_swag_sample_diagonal_bitwise(drift):
    means, diags, _, js, z1, z2 = _sample_inputs(seed=1)
    md = _dev(means)
    th = swag_sample(md, _dev(diags), None, js, z1, z2, drift).cpu().numpy()
    mref = means.copy()
    ref = _sample_np(mref, diags, None, js, z1, z2, drift)
    assert np.array_equal(th, ref, equal_nan=True)
    assert np.array_equal(md.cpu().numpy(), mref if drift else means, equal_nan=True)


def test_swag_sample_deterministic():
    means, diags, D, js, z1, z2 = _sample_inputs(B=9, K=10, p=5000, M=300, seed=2)
    outs = []
    for _ in range(2):
        md = _dev(means)
        outs.append((swag_sample(md, _dev(diags), _dev(D), js, z1, z2, True).cpu().numpy(), md.cpu().numpy()))
    assert np.array_equal(outs[0][0], outs[1][0], equal_nan=True)
    assert np.array_equal(outs[0][1], outs[1][1], equal_nan=True)


def test_swag_refusals():
    W = torch.zeros(2, 5, dtype=torch.float64, device=DEV)
    with pytest.raises(_lib.QuinnAmdError):
        swag_step(7, W, m1=W.clone(), m2=W.clone())
    with pytest.raises(_lib.QuinnAmdError):               # ring slot outside [0, K)
        swag_step(_lib.SWAG_SGD_COLLECT, W, W.clone(), torch.ones(2, dtype=torch.float64, device=DEV), 1.0, W.clone(),
                  W.clone(), torch.zeros(2, 3, 5, dtype=torch.float64, device=DEV), slot=3, n=1)
    with pytest.raises(_lib.QuinnAmdError):               # n < 1
        swag_step(_lib.SWAG_SGD_COLLECT, W, W.clone(), torch.ones(2, dtype=torch.float64, device=DEV), 1.0, W.clone(),
                  W.clone(), None, n=0)
    with pytest.raises(ValueError):                       # member index out of range
        swag_sample(W.clone(), W.clone(), None, [0, 2], np.zeros((2, 5)), np.zeros((2, 2)), True)
    with pytest.raises(_lib.QuinnAmdError):               # K = 1: sqrt(K - 1) = 0
        swag_sample(W.clone(), W.clone(), torch.zeros(2, 1, 5, dtype=torch.float64, device=DEV), [0], np.zeros((1, 5)),
                    np.zeros((1, 1)), True)


# ------------------------------------------------------------------------------------- end to end vs the reference
def _net(g):
    if "rdim" in g:
        return R.RNet(int(g["rdim"]), int(g["nlayers"]), wp_function=R.Poly(int(g["wp_arg"])), indim=int(g["indim"]),
                      outdim=int(g["outdim"]), layer_pre=bool(g["layer_pre"]), layer_post=bool(g["layer_post"]),
                      biasorno=bool(g["biasorno"]), nonlin=bool(g["nonlin"]), mlp=bool(g["mlp"]))
    dims = [int(v) for v in g["dims"]]
    return MLP(dims[0], dims[-1], tuple(dims[1:-1]), activ=str(g["activ"]))


def _fit(g, dtype="float64", **extra):
    net = _net(g)
    load_flat_into(net, g["w0"])
    sw = NN_SWAG(net, nens=int(g["nens"]), dfrac=float(g["dfrac"]), k=int(g["k"]), n_steps=int(g["n_steps"]),
                 c=int(g["c"]), cov_type=str(g["cov_type"]), lr_swag=float(g["lr_swag"]), datanoise=float(g["datanoise"]),
                 verbose=False, dtype=dtype, **extra)
    np.random.seed(int(g["np_seed"]))
    torch.manual_seed(int(g["torch_seed"]))
    kw = dict(lrate=float(g["lrate"]), nepochs=int(g["nepochs"]), batch_size=int(g["batch_size"]) if "batch_size" in g else None)
    sw.fit(g["x"], g["y"], val=[g["xval"], g["yval"]], freq_out=1000, **kw)
    return sw


def _g9(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    np.testing.assert_allclose(a, b, rtol=1e-9, atol=1e-9 * np.max(np.abs(b)), err_msg=what)


@pytest.mark.parametrize("name", ["g15_swag_mlp_lowrank.npz", "g15_swag_mlp_diag.npz", "g15_swag_rnet_lowrank.npz"])
def test_nn_swag_end_to_end_vs_reference(name):
    g = load_golden(name)
    sw = _fit(g)
    assert np.array_equal(sw.rows, g["rows"])
    _g9(sw.fit_results["final_w"], g["traj"][:, 0], "MAP weights")
    _g9(sw.means, g["means"], "means")
    _g9(sw.cov_diags, g["cov_diags"], "cov_diags")
    if str(g["cov_type"]) == "lowrank":
        _g9(sw.d_mats, g["d_mats"], "d_mats")
    else:
        assert sw.d_mats == []
    from quinn_amd.ops import flatten_module
    for j, learner in enumerate(sw.learners):             # the member's module ends at its last SWAG weights
        _g9(flatten_module(learner.nnmodel), g["traj"][j, -1], f"learner {j}")
    thetas = []
    orig = sw._predict_batch_dev
    sw._predict_batch_dev = lambda W, x: (thetas.append(W.cpu().numpy()), orig(W, x))[1]
    np.random.seed(int(g["pred_seed"]))
    for call in range(2):
        thetas.clear()
        y = sw.predict_ens(g["xpred"], nens=int(g["npred"]))
        _g9(thetas[0], g["pred_thetas"][call], f"thetas {call}")
        _g9(y, g["pred"][call], f"pred {call}")
        _g9(sw.means, g["means_after"][call], f"means after {call}")


def test_nn_swag_mean_drift_off_keeps_means():
    g = load_golden("g15_swag_mlp_lowrank.npz")
    sw = _fit(g, mean_drift=False)
    m0 = np.array(sw.means)
    np.random.seed(int(g["pred_seed"]))
    y = sw.predict_ens(g["xpred"], nens=int(g["npred"]))
    assert np.array_equal(np.array(sw.means), m0)
    assert np.isfinite(y).all() and y.shape == g["pred"][0].shape
    # the first draw of each member sees the same mean with and without drift
    _g9(y[0], g["pred"][0][0], "first draw")
    mean, var, _ = sw.predict_mom_sample(g["xpred"], msc=1, nsam=50)
    assert np.isfinite(mean).all() and np.isfinite(var).all()


def test_nn_swag_float32_runs():
    g = load_golden("g15_swag_mlp_lowrank.npz")
    sw = _fit(g, dtype="float32")
    m = np.array(sw.means)
    assert np.isfinite(m).all() and np.isfinite(np.array(sw.d_mats)).all()
    assert np.max(np.abs(m - g["means"])) <= 1e-3 * np.max(np.abs(g["means"]))
    np.random.seed(int(g["pred_seed"]))
    y = sw.predict_ens(g["xpred"], nens=int(g["npred"]))
    assert y.shape == g["pred"][0].shape and np.isfinite(y).all()


def test_ex_ufit_swag_runs():
    path = os.path.join(os.path.dirname(GOLD), "..", "examples", "ex_ufit.py")
    spec = importlib.util.spec_from_file_location("ex_ufit_swag", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    torch.manual_seed(0)
    np.random.seed(0)
    ymean, ystd, rmse = mod.main("swag", quick=True)
    assert np.isfinite(rmse) and np.isfinite(ymean).all() and np.isfinite(ystd).all()
