"""GPU: qn_la_evidence and qn_la_tune (csrc/qn_evidence.hip) against their contract `quinn_amd/evidence.py` in np.longdouble,
and the surface built on them (`NN_Laplace.log_marginal_likelihood` / `tune_hyper` / `evidence_weights`).

The bars are derived, not measured.  Assume every term of a sum is accurate to 4 ulp; a sum of m such terms in any order is then
within (m + 8) eps sum |term| of the exact sum (`sum_bar`).  That gives the bars of logdet (the terms log lambda_j), gamma_g and
gamma ((c_j / s2) / lambda_j), S_g (w_j^2) and loglik (its two terms) directly; logZ is the sum of loglik, the G terms
n_g/2 log tau_g, the G terms -tau_g S_g / 2 and -logdet / 2, so its bar is the bars of those terms (4 ulp for a term that is no
sum itself) plus (2 G + 2 + 8) eps sum |term|.  `row_bars` computes all of them from the longdouble contract.
The randomised grids keep tau >= 3, so that no log lambda_j is near 0: there "4 ulp of the term" cannot hold for any float64
evaluation of log(c_j / s2 + tau), because the rounding of lambda_j alone is an absolute error of about eps in its log."""
import numpy as np
import pytest
import torch

from quinn_amd import _lib, evidence as ev
from test_la_evidence_cpu import CONVERGING, FALLBACK, LD, S2_0

pytestmark = pytest.mark.gpu
EPS = float(np.finfo(np.float64).eps)
NO = len(ev.ROWS)


def cuda(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def sum_bar(terms):
    return (len(terms) + 8) * EPS * float(np.sum(np.abs(terms)))


def row_bars(c, bounds, W, sse, n, s2, tau):
    """(rows, bars) `[4 + 2 G]` of one member at one candidate: the contract in longdouble and the module docstring's bars."""
    G = len(bounds) - 1
    rows = ev.log_evidence(c, bounds, W, sse, n, s2, tau, dtype=LD)
    c, W, tau, s2, sse = np.asarray(c, dtype=LD), np.asarray(W, dtype=LD), np.asarray(tau, dtype=LD), LD(s2), LD(sse)
    a = c / s2
    lam = a + np.repeat(tau, np.diff(bounds))
    bars = np.empty(NO + 2 * G)
    bars[2] = sum_bar(np.log(lam))
    bars[3] = sum_bar(a / lam)
    for g, (lo, hi) in enumerate(zip(bounds[:-1], bounds[1:])):
        bars[NO + g] = sum_bar((a / lam)[lo:hi])
        bars[NO + G + g] = sum_bar((W * W)[lo:hi])
    two_pi = LD(8) * np.arctan(LD(1))
    bars[1] = sum_bar([-LD(0.5) * n * np.log(two_pi * s2), -LD(0.5) * sse / s2])
    ng = np.diff(bounds).astype(LD)
    pri, quad = LD(0.5) * ng * np.log(tau), -LD(0.5) * tau * rows[NO + G:]
    terms = np.concatenate([[rows[1]], pri, quad, [-LD(0.5) * rows[2]]])
    bars[0] = bars[1] + 4 * EPS * float(np.sum(np.abs(pri))) + float(np.sum(0.5 * tau * bars[NO + G:] + 4 * EPS * np.abs(quad))) + \
        0.5 * bars[2] + sum_bar(terms)
    return rows, bars


def assert_rows(got, c, bounds, W, sse, n, s2, tau, what):
    ref, bars = row_bars(c, bounds, W, sse, n, s2, tau)
    err = np.abs(got.astype(LD) - ref).astype(np.float64)
    print(f"{what}: max err / bar {float(np.max(err / np.maximum(bars, 1e-300))):.3f} (logZ {float(ref[0]):.6g}, err {err[0]:.2e}, bar {bars[0]:.2e})")
    assert np.all(err <= bars), (what, err / bars)


def make_bounds(p, G, seed):
    """G groups of p elements, the first of one element where there is room."""
    rs = np.random.RandomState(seed)
    if G == 1:
        return np.array([0, p], dtype=np.int64)
    inner = 1 + np.sort(rs.permutation(np.arange(1, p - 1))[:G - 2]) if G > 2 else np.array([], dtype=np.int64)
    return np.r_[0, 1, inner, p].astype(np.int64)


def grid_case(p, G, B=5, Hc=4, seed=0):
    rs = np.random.RandomState(1000 * p + 10 * G + seed)
    bounds = make_bounds(p, G, p + G)
    c = np.exp(rs.randn(B, p) * 2.0 + 1.0) * (rs.rand(B, p) < 0.8)
    W = 0.5 * rs.randn(B, p)
    sse = 0.01 * rs.chisquare(64, size=B)
    s2 = np.exp(rs.uniform(np.log(1e-3), np.log(0.05), size=(B, Hc)))
    tau = np.exp(rs.uniform(np.log(3.0), np.log(300.0), size=(B, Hc, G)))
    return bounds, c, W, sse, s2, tau


SHAPES = [(p, G) for p in (1, 54, 255, 256, 257, 1031) for G in (1, 3, 32) if G <= p]


# ------------------------------------------------------------------------------------------ qn_la_evidence
@pytest.mark.parametrize("p,G", SHAPES)
def test_evidence_equals_contract_and_bits_do_not_depend_on_B_or_Hc(p, G):
    B, Hc, n = 5, 4, 64
    bounds, c, W, sse, s2, tau = grid_case(p, G, B, Hc)
    assert G == 1 or bounds[1] == 1                             # a group of one element
    out = ev.log_evidence_dev(cuda(c), cuda(W), cuda(sse), n, bounds, cuda(s2), cuda(tau)).cpu().numpy()
    assert out.shape == (B, Hc, NO + 2 * G)
    for b in range(B):
        for h in range(Hc):
            assert_rows(out[b, h], c[b], bounds, W[b], sse[b], n, s2[b, h], tau[b, h], f"p={p} G={G} b={b} h={h}")
    again = ev.log_evidence_dev(cuda(c), cuda(W), cuda(sse), n, bounds, cuda(s2), cuda(tau)).cpu().numpy()
    assert np.array_equal(out, again)
    b, h = 2, 3
    one = ev.log_evidence_dev(cuda(c[b:b + 1]), cuda(W[b:b + 1]), cuda(sse[b:b + 1]), n, bounds, cuda(s2[b:b + 1]),
                              cuda(tau[b:b + 1])).cpu().numpy()
    assert np.array_equal(one[0], out[b])
    one = ev.log_evidence_dev(cuda(c[b:b + 1]), cuda(W[b:b + 1]), cuda(sse[b:b + 1]), n, bounds, cuda(s2[b:b + 1, h:h + 1]),
                              cuda(tau[b:b + 1, h:h + 1])).cpu().numpy()
    assert np.array_equal(one[0, 0], out[b, h])


def test_evidence_nan_isolation():
    p, G, B, Hc, n = 257, 3, 5, 4, 64
    bounds, c, W, sse, s2, tau = grid_case(p, G, B, Hc)
    clean = ev.log_evidence_dev(cuda(c), cuda(W), cuda(sse), n, bounds, cuda(s2), cuda(tau)).cpu().numpy()
    assert np.all(np.isfinite(clean))
    s2b, taub, cb, Wb, sseb = s2.copy(), tau.copy(), c.copy(), W.copy(), sse.copy()
    s2b[0, 1] = -1.0                    # one bad candidate each ...
    s2b[0, 2] = np.inf
    taub[1, 0, 2] = 0.0
    taub[1, 3, 0] = np.nan
    cb[2, 256] = -1e-300                # ... and one bad element each (the last of member 2: the one wave 0 holds alone)
    Wb[3, 100] = np.inf
    sseb[4] = np.nan
    out = ev.log_evidence_dev(cuda(cb), cuda(Wb), cuda(sseb), n, bounds, cuda(s2b), cuda(taub)).cpu().numpy()
    nan = np.zeros((B, Hc), dtype=bool)
    nan[0, 1] = nan[0, 2] = nan[1, 0] = nan[1, 3] = True
    nan[2:] = True
    assert np.all(np.isnan(out[nan])) and np.array_equal(out[~nan], clean[~nan])
    cb = c.copy()
    cb[2, 5] = np.nan
    out = ev.log_evidence_dev(cuda(cb), cuda(W), cuda(sse), n, bounds, cuda(s2), cuda(tau)).cpu().numpy()
    assert np.all(np.isnan(out[2])) and np.array_equal(np.delete(out, 2, axis=0), np.delete(clean, 2, axis=0))


# ------------------------------------------------------------------------------------------ qn_la_tune
def dev_tune(c, bounds, W, sse, n, s2_0, tau_0, **kw):
    """`tune_dev` on numpy members c, W [B, p] -> numpy dict."""
    res = ev.tune_dev(cuda(c), cuda(W), cuda(sse), n, bounds, cuda(s2_0), cuda(tau_0), **kw)
    return {k: v.cpu().numpy() for k, v in res.items()}


def status_of(res, b=0):
    return dict(zip(ev.STATUS, res["status"][b]))


@pytest.mark.parametrize("p,G", [(1, 1), (54, 3), (257, 32), (1031, 3)])
def test_tune_max_iter_0_returns_the_start(p, G):
    B, n = 5, 64
    bounds, c, W, sse, s2, tau = grid_case(p, G, B, 1, seed=1)
    s2, tau = s2[:, 0], tau[:, 0]
    res = dev_tune(c, bounds, W, sse, n, s2, tau, max_iter=0, tol=0.0)
    assert np.array_equal(res["s2"], s2) and np.array_equal(res["tau"], tau)
    for b in range(B):
        assert_rows(res["rows"][b], c[b], bounds, W[b], sse[b], n, s2[b], tau[b], f"p={p} G={G} b={b}")
        ref = ev.tune(c[b], bounds, W[b], sse[b], n, s2[b], tau[b], max_iter=0, tol=0.0, dtype=LD)
        st = status_of(res, b)
        assert st["iters"] == ref["iters"] == 0 and st["returned"] == 0 and st["converged"] == ref["converged"] == 0
        assert st["clamped"] == 0 and st["logZ_start"] == res["rows"][b, 0]
        # resid is the largest |log| of a quotient of two sums: their relative bars, and a few roundings
        rows, bars = row_bars(c[b], bounds, W[b], sse[b], n, s2[b], tau[b])
        if np.isfinite(float(ref["resid"])):
            slack = float(np.max(bars[NO:NO + G] / rows[NO:NO + G] + bars[NO + G:] / rows[NO + G:]) + bars[3] / abs(n - rows[3])) + 8 * EPS
            assert abs(st["resid"] - float(ref["resid"])) <= slack * max(1.0, float(ref["resid"])), (st["resid"], ref["resid"])
        else:
            assert st["resid"] == np.inf


@pytest.mark.parametrize("name", list(CONVERGING))
def test_tune_converges_with_a_certificate(name):
    p, G, n, nz, seed = CONVERGING[name]
    tol, cov_scale = 1e-10, 0.7
    c, bounds, W, sse = ev.synthetic_member(p, G, n, nz, seed)
    args = (c[None], bounds, W[None], np.array([sse]), n, np.array([S2_0]), np.ones((1, G)))
    res = dev_tune(*args, tol=tol, cov_scale=cov_scale, want_dinv=True)
    st = status_of(res)
    print(f"{name}: iters {st['iters']:.0f} resid {st['resid']:.3e} logZ {st['logZ_start']:.6g} -> {res['rows'][0, 0]:.6g}")
    assert st["converged"] == 1 and st["returned"] == st["iters"] <= 20 and st["clamped"] == 0 and st["resid"] <= tol
    s2, tau = res["s2"][0], res["tau"][0]
    rows, bars = row_bars(c, bounds, W, sse, n, s2, tau)
    # the certificate: the stopping rule re-evaluated by the contract at the DEVICE's answer
    share = float(np.max(bars[NO:NO + G] / rows[NO:NO + G] + bars[NO + G:] / rows[NO + G:]) + bars[3] / abs(n - rows[3]))
    assert float(ev.residual(rows, G, LD(sse), n, LD(s2), tau.astype(LD))) <= tol + share
    assert_rows(res["rows"][0], c, bounds, W, sse, n, s2, tau, name)
    assert res["rows"][0, 0] >= st["logZ_start"]
    lam = np.asarray(c, dtype=LD) / LD(s2) + np.repeat(tau.astype(LD), np.diff(bounds))
    for key, want in (("Dinv", 1 / (LD(cov_scale) * lam)), ("Dih", np.sqrt(1 / (LD(cov_scale) * lam)))):
        ulps = np.abs(res[key][0].astype(LD) - want).astype(np.float64) / np.spacing(want.astype(np.float64))
        print(f"  {key}: max {ulps.max():.2f} ulp")
        assert np.all(ulps <= 2.0), key
    again = dev_tune(*args, tol=tol, cov_scale=cov_scale, want_dinv=True)
    for key in res:
        assert np.array_equal(res[key], again[key]), key
    # inside a batch of other members: the same bits
    c2, b2, W2, sse2 = ev.synthetic_member(p, G, n, nz, seed + 100)
    both = dev_tune(np.stack([c2, c]), bounds, np.stack([W2, W]), np.array([sse2, sse]), n, np.full(2, S2_0), np.ones((2, G)), tol=tol,
                    cov_scale=cov_scale, want_dinv=True)
    for key in res:
        assert np.array_equal(res[key][0], both[key][1]), key


@pytest.mark.parametrize("name", list(FALLBACK))
def test_tune_fallback(name):
    p, G, n, seed, log_mean = FALLBACK[name]
    c, bounds, W, sse = ev.synthetic_member(p, G, n, None, seed, log_mean=log_mean)
    clamps = dict(s2_min=1e-6, s2_max=10.0, tau_min=1e-3, tau_max=1e3)
    ref = ev.tune(c, bounds, W, sse, n, S2_0, np.ones(G), tol=1e-10, max_iter=200, **clamps)
    res = dev_tune(c[None], bounds, W[None], np.array([sse]), n, np.array([S2_0]), np.ones((1, G)), tol=1e-10, max_iter=200, **clamps)
    st = status_of(res)
    print(f"{name}: returned {st['returned']:.0f} (contract {ref['returned']}) logZ {st['logZ_start']:.6g} -> {res['rows'][0, 0]:.6g} "
          f"(contract {float(ref['rows'][0]):.6g}) clamped {st['clamped']:.0f}")
    assert st["converged"] == 0 and st["iters"] == 200 and res["rows"][0, 0] >= st["logZ_start"]
    assert clamps["s2_min"] <= res["s2"][0] <= clamps["s2_max"]
    assert np.all((res["tau"][0] >= clamps["tau_min"]) & (res["tau"][0] <= clamps["tau_max"]))
    _, bars = row_bars(c, bounds, W, sse, n, ref["s2"], ref["tau"])
    assert abs(res["rows"][0, 0] - float(ref["rows"][0])) <= bars[0]
    assert_rows(res["rows"][0], c, bounds, W, sse, n, res["s2"][0], res["tau"][0], name)     # the rows belong to the answer
    if name != "wanders":
        assert int(st["clamped"]) & ev.CLAMP_S2_MAX


def test_tune_untuned_components_keep_their_bits():
    p, G, n, nz, seed = CONVERGING["p54_n64"]
    c, bounds, W, sse = ev.synthetic_member(p, G, n, nz, seed)
    s2_0, tau_0 = np.array([0.123]), np.array([[0.3, 1.7, 2.9]])
    args = (c[None], bounds, W[None], np.array([sse]), n, s2_0, tau_0)
    res = dev_tune(*args, tune_noise=False)
    assert np.array_equal(res["s2"], s2_0) and status_of(res)["converged"] == 1 and not np.array_equal(res["tau"], tau_0)
    res = dev_tune(*args, tune_prior=False)
    assert np.array_equal(res["tau"], tau_0) and status_of(res)["converged"] == 1 and res["s2"][0] != s2_0[0]
    res = dev_tune(*args, tune_noise=False, tune_prior=False)
    st = status_of(res)
    assert np.array_equal(res["s2"], s2_0) and np.array_equal(res["tau"], tau_0) and st["iters"] == 0 and st["converged"] == 1
    assert st["resid"] == 0.0
    # a member with a bad element: NaN rows, its start back, nothing else touched
    cb = np.stack([c, c])
    cb[0, 7] = -1.0
    res = dev_tune(cb, bounds, np.stack([W, W]), np.array([sse, sse]), n, np.full(2, 0.123), np.repeat(tau_0, 2, axis=0), want_dinv=True)
    good = dev_tune(*args, want_dinv=True)
    assert np.all(np.isnan(res["rows"][0])) and np.all(np.isnan(res["Dinv"][0])) and res["s2"][0] == 0.123
    assert status_of(res, 0)["converged"] == 0 and status_of(res, 0)["resid"] == np.inf
    for key in good:
        assert np.array_equal(res[key][1], good[key][0]), key


# ------------------------------------------------------------------------------------------ NN_Laplace
def _data():
    rs = np.random.RandomState(7)
    x = rs.rand(96, 3) * 2 - 1
    y = np.stack([np.sin(2 * x[:, 0]) + x[:, 1], x[:, 2] ** 2 - x[:, 0]], axis=1) + 0.1 * rs.randn(96, 2)
    return x[:64], y[:64], x[64:], y[64:]


GROUPS = {"kron": "layer", "ggn_diag": "tensor", "ggn": "all"}


@pytest.mark.parametrize("la_type", list(GROUPS))
def test_nn_laplace_end_to_end(la_type, monkeypatch):
    from quinn_amd.nns.mlp import MLP
    from quinn_amd.ops import BatchedMLP
    from quinn_amd.solvers import NN_Laplace
    from quinn_amd.solvers.nn_laplace import glm_mixture
    torch.manual_seed(0)
    np.random.seed(0)
    xtrn, ytrn, xtst, ytst = _data()
    sse_calls = []
    real_sse = BatchedMLP.sse
    monkeypatch.setattr(BatchedMLP, "sse", lambda self, W, row_idx=None: (sse_calls.append(1), real_sse(self, W, row_idx))[1])
    la = NN_Laplace(MLP(3, 2, (5, 4), biasorno=True, activ='tanh').double(), la_type=la_type, nens=3, dfrac=0.8, datanoise=0.3,
                    priorsigma=2.0, verbose=False)
    la.fit(xtrn, ytrn, val=[xtst, ytst], lrate=0.01, batch_size=16, nepochs=40, freq_out=1000)
    base = len(sse_calls)
    la.predict_glm(xtst, msc=1, noise=True)
    before = la.score_glm(xtst, ytst)
    assert len(sse_calls) == base and la._ev_cache is None and la.datanoise_ is None        # an untouched solver: nothing new runs
    p, nens = la.nparams, 3
    assert la.arch.dims == (3, 5, 4, 2) and p == 54
    # ---- the evidence at the fit's scales against the contract fed the device's spectrum
    lml = la.log_marginal_likelihood()
    assert lml.shape == (nens,) and len(sse_calls) == base + 1
    c, W, sse, n = la._evidence_inputs()
    c, W, sse = c.cpu().numpy(), W.cpu().numpy(), sse.cpu().numpy()
    assert n == 51 * 2 and c.shape == (nens, p) and np.all(c >= 0) and np.array_equal(W, np.asarray(la.means))
    s2, tau = 0.3 ** 2, 1.0 / 2.0 ** 2
    for j in range(nens):
        ref, bars = row_bars(c[j], np.array([0, p]), W[j], sse[j], n, s2, [tau])
        assert abs(lml[j] - float(ref[0])) <= bars[0], (j, lml[j], ref[0])
        loglik = -0.5 * n * np.log(2 * np.pi * s2) - 0.5 * sse[j] / s2
        if la_type == 'ggn':
            logdet = np.linalg.slogdet(la.hessians[j])[1]
        elif la_type == 'kron':
            logdet = -(np.linalg.slogdet(la.dense_cov(j))[1] + p * np.log(la.cov_scale))
        else:
            logdet = float(np.sum(np.log(np.diag(la.hessians[j]))))
        direct = loglik + 0.5 * p * np.log(tau) - 0.5 * tau * np.sum(W[j] ** 2) - 0.5 * logdet
        assert abs(lml[j] - direct) <= 1e-9 * abs(direct), (j, lml[j], direct)
    assert len(sse_calls) == base + 1                                                        # the SSE is cached
    full = la.log_marginal_likelihood(full=True)
    assert np.array_equal(full["logZ"], lml) and full["gamma_g"].shape == (nens, 1) and np.all(full["gamma"] < p)
    # ---- a grid: [nens, Hc], and the column at the fit's own scales is the no-argument call bit for bit
    grid = la.log_marginal_likelihood(datanoise=[0.1, 0.3, 1.0], priorsigma=[1.0, 2.0, 4.0])
    assert grid.shape == (nens, 3) and np.array_equal(grid[:, 1], lml)
    G = len(ev.group_bounds(la.arch, GROUPS[la_type])[0]) - 1
    grid = la.log_marginal_likelihood(datanoise=[0.1, 0.3], priorsigma=np.full((2, G), 2.0), groups=GROUPS[la_type])
    assert grid.shape == (nens, 2) and np.all(np.abs(grid[:, 1] - lml) <= 1e-12 * np.maximum(1.0, np.abs(lml)))
    w = la.evidence_weights()
    assert w.shape == (nens,) and abs(w.sum() - 1) < 1e-14 and np.all(w >= 0)
    # ---- empirical Bayes
    dry = la.tune_hyper(groups=GROUPS[la_type], apply=False)
    assert la.datanoise_ is None and la._ev_logZ is not None
    if G == 1:
        assert np.array_equal(dry["logZ_start"], lml)
    res = la.tune_hyper(groups=GROUPS[la_type])
    print(la_type, "logZ", res["logZ_start"], "->", res["logZ"], "datanoise", res["datanoise"], "iters", res["iters"],
          "converged", res["converged"])
    assert np.all(res["logZ"] >= res["logZ_start"]) and res["prior_prec"].shape == (nens, G) and len(res["prior_groups"]) == G
    assert np.array_equal(res["logZ"], dry["logZ"]) and np.array_equal(la.datanoise_, res["datanoise"])
    assert la.datanoise == 0.3 and la.priorsigma == 2.0 and np.array_equal(la.prior_prec_, res["prior_prec"])
    s2t, taut = res["datanoise"] ** 2, res["prior_prec"]
    for j in range(nens):
        if la_type == 'kron':
            k = la.kron[j]
            for i in range(3):
                want = 1.0 / (la.cov_scale * (k["lamS"][i][:, None] * k["lamA"][i][None, :] / (k["nb"] * s2t[j]) + taut[j, i]))
                assert torch.allclose(k["Dinv"][i], want, rtol=1e-13, atol=0.0)
        elif la_type == 'ggn_diag':
            bounds = ev.group_bounds(la.arch, 'tensor')[0]
            want = 1.0 / (la.cov_scale * (c[j] / s2t[j] + np.repeat(taut[j], np.diff(bounds))))
            np.testing.assert_allclose(np.diag(la.cov_mats[j]), want, rtol=1e-13)
        else:
            H = la._G_dev[j].cpu().numpy() / s2t[j] + taut[j, 0] * np.eye(p)
            np.testing.assert_allclose(la.cov_mats[j] @ (la.cov_scale * H), np.eye(p), atol=1e-9)
    w = la.evidence_weights()
    assert abs(w.sum() - 1) < 1e-14 and np.array_equal(w, ev.softmax_weights(res["logZ"]))
    # ---- the predictives use the tuned scales; a scalar noise= is the plain mixture formula
    ym, yv, _ = la.predict_glm(xtst, msc=1, noise=True)
    f, S = la._glm_members(xtst)
    f, S = f.cpu().numpy(), S.cpu().numpy()
    _, cov = glm_mixture(f, S, la.datanoise_ ** 2)
    assert np.allclose(yv, np.stack([cov[:, 0, 0], cov[:, 1, 1]], axis=1), rtol=1e-13)
    assert np.allclose(cov, glm_mixture(f, S, float(np.mean(la.datanoise_ ** 2)))[1], rtol=1e-13)

    def nlpd(noise_var):                                        # [M] or scalar: the equal-weight mixture of the members' Gaussians
        V = np.stack([S[:, :, 0, 0], S[:, :, 1, 1]], axis=-1) + np.reshape(noise_var, (-1, 1, 1))
        ll = -0.5 * (ytst[None] - f) ** 2 / V - 0.5 * np.log(2 * np.pi * V)
        return -float(np.mean(np.log(np.mean(np.exp(ll), axis=0))))
    after = la.score_glm(xtst, ytst)
    print(la_type, "nlpd", before["nlpd"], "->", after["nlpd"])
    assert abs(after["nlpd"] - nlpd(la.datanoise_ ** 2)) <= 1e-10 * abs(after["nlpd"])
    assert abs(la.score_glm(xtst, ytst, noise=0.2)["nlpd"] - nlpd(0.04)) <= 1e-10 * abs(nlpd(0.04))
    assert la.predict_ens(xtst, nens=4).shape == (4, 32, 2)
    sc = la.score(xtst, ytst, nsam=nens, member_weights=w, noise=0.3)
    assert np.isfinite(sc["nlpd"])
