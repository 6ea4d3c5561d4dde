"""CPU: the numpy contract of the Laplace evidence (quinn_amd/evidence.py) against closed forms, the fixed point's stationarity,
its fallback and clamps, the argument errors of the Python layer and the refusals of the C entry points (no device needed)."""
import ctypes

import numpy as np
import pytest

from quinn_amd import _lib, evidence as ev
from quinn_amd.ops import MLPArch

LD = np.longdouble
# (p, G, n, non-zero c_j, seed): fewer non-zero c_j than n, the fixed point converges
CONVERGING = {"p54_n64": (54, 3, 64, 30, 1), "p54_n256": (54, 3, 256, 54, 2), "p500_G4": (500, 4, 2000, 300, 3),
              "p500_G1": (500, 1, 2000, 500, 4)}
# more non-zero c_j than n: (p, G, n, seed, log_mean) -- the first wanders without meeting tol, the second and third drive
# n - gamma negative (the third at the start)
FALLBACK = {"wanders": (54, 3, 40, 2, -2.0), "clamps": (54, 3, 40, 3, -2.0), "n_below_gamma": (8513, 4, 4096, 5, 1.0)}
S2_0 = 0.09


def test_exact_on_a_linear_model():
    """y = X~ w + noise with the exact ridge solution: the Laplace evidence is the Gaussian marginal N(y; 0, s2 I + X~ X~^T / tau)."""
    rs = np.random.RandomState(0)
    N, d = 40, 3
    Xt = np.concatenate([rs.randn(N, d), np.ones((N, 1))], axis=1)
    y = Xt @ rs.randn(d + 1) + 0.2 * rs.randn(N)
    c = np.clip(np.linalg.eigvalsh(Xt.T @ Xt), 0.0, None)
    for s2, tau in ((0.04, 1.0), (0.5, 0.1), (0.01, 25.0)):
        w = np.linalg.solve(Xt.T @ Xt / s2 + tau * np.eye(d + 1), Xt.T @ y / s2)
        sse = float(np.sum((y - Xt @ w) ** 2))
        got = ev.log_evidence(c, [0, d + 1], w, sse, N, s2, [tau])[0]
        K = s2 * np.eye(N) + Xt @ Xt.T / tau
        want = -0.5 * (N * np.log(2.0 * np.pi) + np.linalg.slogdet(K)[1] + y @ np.linalg.solve(K, y))
        assert abs(got - want) <= 1e-10 * abs(want), (s2, tau, got, want)


def test_kron_logdet():
    """`kron_spectrum` on dims (3, 5, 2): logdet equals slogdet of blockdiag((S_i kron A_i) / (nb s2) + tau_i I)."""
    rs = np.random.RandomState(1)
    arch = MLPArch((3, 5, 2), "tanh")
    nb, s2, tau = 17, 0.3, np.array([0.7, 2.5])
    e, h = (4, 6), (5, 2)
    A = [(lambda m: m @ m.T)(rs.randn(k, k + 2)) for k in e]
    S = [(lambda m: m @ m.T)(rs.randn(k, k + 2)) for k in h]
    c = ev.kron_spectrum([np.linalg.eigvalsh(s) for s in S], [np.linalg.eigvalsh(a) for a in A], nb)
    bounds, names = ev.group_bounds(arch, 'layer')
    assert c.shape == (arch.nparams,) and list(bounds) == [0, 20, 32] and names == ['layer0', 'layer1']
    rows = ev.log_evidence(c, bounds, np.zeros(arch.nparams), 1.0, 10, s2, tau)
    want = sum(np.linalg.slogdet(np.kron(S[i], A[i]) / (nb * s2) + tau[i] * np.eye(h[i] * e[i]))[1] for i in range(2))
    assert abs(rows[2] - want) <= 1e-10 * abs(want)
    # batched factors give the same numbers member by member
    cb = ev.kron_spectrum([np.stack([np.linalg.eigvalsh(s)] * 2) for s in S], [np.stack([np.linalg.eigvalsh(a)] * 2) for a in A], nb)
    assert cb.shape == (2, arch.nparams) and np.array_equal(cb[0], c) and np.array_equal(cb[1], c)


@pytest.mark.parametrize("name", list(CONVERGING))
def test_stationarity(name):
    p, G, n, nz, seed = CONVERGING[name]
    tol = 1e-10
    c, bounds, W, sse = ev.synthetic_member(p, G, n, nz, seed)
    r = ev.tune(c, bounds, W, sse, n, S2_0, np.ones(G), tol=tol)
    assert r["converged"] == 1 and r["returned"] == r["iters"] <= 20 and r["clamped"] == 0
    s2, tau = float(r["s2"]), np.asarray(r["tau"], dtype=np.float64)
    rows = ev.log_evidence(c, bounds, W, sse, n, s2, tau, dtype=LD)
    assert float(ev.residual(rows, G, LD(sse), n, LD(s2), tau.astype(LD))) <= tol
    logZ, h = float(rows[0]), 1e-4

    def at(ds, dt):
        return float(ev.log_evidence(c, bounds, W, sse, n, LD(s2) * np.exp(LD(ds)), tau.astype(LD) * np.exp(dt.astype(LD)), dtype=LD)[0])
    zero = np.zeros(G)
    assert abs(at(h, zero) - at(-h, zero)) / (2 * h) <= 1e-5 * abs(logZ)
    for g in range(G):
        dt = zero.copy()
        dt[g] = h
        assert abs(at(0.0, dt) - at(0.0, -dt)) / (2 * h) <= 1e-5 * abs(logZ), g
    assert logZ >= float(r["logZ_start"])


@pytest.mark.parametrize("name", list(FALLBACK))
def test_fallback_and_clamps(name):
    p, G, n, seed, log_mean = FALLBACK[name]
    c, bounds, W, sse = ev.synthetic_member(p, G, n, None, seed, log_mean=log_mean)
    clamps = dict(s2_min=1e-6, s2_max=10.0, tau_min=1e-3, tau_max=1e3)
    r = ev.tune(c, bounds, W, sse, n, S2_0, np.ones(G), tol=1e-10, max_iter=200, trace=True, **clamps)
    assert r["converged"] == 0 and r["iters"] == 200 and len(r["logZs"]) == 201
    assert r["rows"][0] >= r["logZ_start"] == r["logZs"][0]
    finite = np.where(np.isfinite(r["logZs"]), r["logZs"], -np.inf)
    assert r["returned"] == int(np.argmax(finite)) and r["rows"][0] == finite.max()          # the first of the largest
    assert clamps["s2_min"] <= r["s2"] <= clamps["s2_max"]
    assert np.all((r["tau"] >= clamps["tau_min"]) & (r["tau"] <= clamps["tau_max"]))
    np.testing.assert_array_equal(r["rows"], ev.log_evidence(c, bounds, W, sse, n, r["s2"], r["tau"]))
    if name == "wanders":
        assert r["returned"] > 0 and r["rows"][0] > r["logZ_start"]
    if name == "clamps":
        assert r["clamped"] & ev.CLAMP_S2_MAX and r["returned"] > 0
    if name == "n_below_gamma":
        assert ev.log_evidence(c, bounds, W, sse, n, S2_0, np.ones(G))[3] > n and r["resids"][0] == np.inf        # at the start
        assert r["clamped"] & ev.CLAMP_S2_MAX


def test_untuned_components_keep_their_bits_and_nan_rules():
    c, bounds, W, sse = ev.synthetic_member(54, 3, 64, 30, 1)
    tau0 = np.array([0.3, 1.7, 2.9])
    r = ev.tune(c, bounds, W, sse, 64, 0.123, tau0, tune_noise=False)
    assert r["s2"] == 0.123 and r["converged"] == 1 and not np.array_equal(r["tau"], tau0)
    r = ev.tune(c, bounds, W, sse, 64, 0.123, tau0, tune_prior=False)
    assert np.array_equal(r["tau"], tau0) and r["converged"] == 1 and r["s2"] != 0.123
    r = ev.tune(c, bounds, W, sse, 64, 0.123, tau0, tune_noise=False, tune_prior=False)
    assert r["iters"] == 0 and r["converged"] == 1 and r["resid"] == 0
    for bad in (dict(s2=-1.0), dict(s2=np.inf), dict(tau=[1.0, 0.0, 1.0]), dict(sse=np.nan)):
        kw = dict(sse=sse, s2=0.1, tau=tau0)
        kw.update(bad)
        assert np.all(np.isnan(ev.log_evidence(c, bounds, W, kw["sse"], 64, kw["s2"], kw["tau"])))
    cb = np.stack([c, c])
    cb[1, 7] = -1e-3
    rows = ev.log_evidence(cb, bounds, W, sse, 64, 0.1, tau0)
    assert np.all(np.isfinite(rows[0])) and np.all(np.isnan(rows[1]))
    r = ev.tune(cb[1], bounds, W, sse, 64, 0.1, tau0)
    assert np.all(np.isnan(r["rows"])) and r["converged"] == 0 and r["iters"] == 0 and r["resid"] == np.inf and r["s2"] == 0.1


def test_python_layer_argument_errors():
    from quinn_amd.nns.mlp import MLP
    from quinn_amd.solvers.nn_laplace import NN_Laplace
    with pytest.raises(ValueError, match="eigenbasis"):
        ev.check_groups('kron', 'tensor')
    with pytest.raises(ValueError, match="commute"):
        ev.check_groups('ggn', 'layer')
    for la_type in ('full', 'diag'):
        with pytest.raises(ValueError, match="hard-wired"):
            ev.check_groups(la_type, 'all')
    with pytest.raises(ValueError):
        ev.check_groups('ggn_diag', 'rows')
    for groups in ('layer', 'tensor', 'all'):
        ev.check_groups('ggn_diag', groups)
    cases = (('kron', dict(groups='tensor')), ('ggn', dict(groups='layer')), ('ggn', dict(groups='tensor')), ('full', {}), ('diag', {}))
    for la_type, kw in cases:
        la = NN_Laplace(MLP(3, 2, (5, 4), activ='tanh'), la_type=la_type, nens=2, device='cpu')
        for method in (la.log_marginal_likelihood, la.tune_hyper):
            with pytest.raises(ValueError):
                method(**kw)
    la = NN_Laplace(MLP(3, 2, (5, 4), activ='tanh'), la_type='full', nens=2, device='cpu')
    with pytest.raises(ValueError):
        la.evidence_weights()
    with pytest.raises(ValueError):
        ev.softmax_weights([np.nan, -np.inf])
    w = ev.softmax_weights([-1000.0, -1001.0, np.nan])
    assert w[2] == 0 and abs(w.sum() - 1) < 1e-15 and abs(w[0] / w[1] - np.e) < 1e-12
    with pytest.raises(ValueError):
        ev.tune(np.ones(4), [0, 4], np.ones(4), 1.0, 10, 0.1, [1.0], max_iter=ev.MAX_ITER + 1)
    with pytest.raises(ValueError):
        ev.log_evidence(np.ones(4), [0, 2, 2, 4], np.ones(4), 1.0, 10, 0.1, [1.0, 1.0, 1.0])


def test_workspace_queries_and_refusals_without_a_device():
    _lib.build()
    L = _lib.lib()
    assert _lib.EV_NOUT == 4 and _lib.EV_NSTATUS == len(ev.STATUS) and _lib.EV_MAX_G == 32 and _lib.EV_MAX_ITER == ev.MAX_ITER
    assert (_lib.EV_CLAMP_S2_MIN, _lib.EV_CLAMP_S2_MAX, _lib.EV_CLAMP_TAU_MIN, _lib.EV_CLAMP_TAU_MAX) == \
        (ev.CLAMP_S2_MIN, ev.CLAMP_S2_MAX, ev.CLAMP_TAU_MIN, ev.CLAMP_TAU_MAX)
    for name in ("qn_la_evidence", "qn_la_evidence_workspace_bytes", "qn_la_tune", "qn_la_tune_workspace_bytes"):
        assert name in _lib.EV_FUNCTIONS and name not in _lib.SYMBOLS and hasattr(L, name)
    assert L.qn_la_evidence_workspace_bytes(5, 1031, 32, 4) >= 33 * 8
    assert L.qn_la_tune_workspace_bytes(512, 200000, 4) >= 5 * 8
    assert L.qn_la_evidence_workspace_bytes(1, 1, 1, 1) > 0
    for args in ((0, 10, 1, 1), (1, 0, 1, 1), (1, 10, 0, 1), (1, 10, 33, 1), (1, 10, 11, 1), (1, 10, 1, 0), (1 << 20, 10, 1, 1 << 12),
                 (1, (1 << 40) + 1, 1, 1)):
        assert L.qn_la_evidence_workspace_bytes(*args) == 0, args
        assert b"qn_la_evidence_workspace_bytes" in L.qn_last_error()
    for args in ((0, 10, 1), (1, 0, 1), (1, 10, 33), (1, 3, 4)):
        assert L.qn_la_tune_workspace_bytes(*args) == 0, args
    EINVAL, EWORKSPACE = _lib.CONSTANTS["QN_EINVAL"], _lib.CONSTANTS["QN_EWORKSPACE"]
    buf = (ctypes.c_double * 64)()                     # never read or written: every call below is refused first
    ptr = ctypes.addressof(buf)
    good = (ctypes.c_int64 * 3)(0, 4, 10)
    need = L.qn_la_evidence_workspace_bytes(2, 10, 2, 1)

    def evidence(n=5, B=2, p=10, bounds=good, G=2, Hc=1, c=ptr, out=ptr, ws=ptr, ws_bytes=need):
        return L.qn_la_evidence(c, ptr, ptr, n, B, p, bounds, G, Hc, ptr, ptr, out, ws, ws_bytes, None)
    assert evidence(n=0) == EINVAL and evidence(B=0) == EINVAL and evidence(G=33) == EINVAL and evidence(Hc=0) == EINVAL
    assert evidence(c=None) == EINVAL and evidence(out=None) == EINVAL and evidence(bounds=None) == EINVAL and evidence(ws=None) == EINVAL
    assert b"NULL" in L.qn_last_error()
    assert evidence(ws_bytes=8) == EWORKSPACE
    for bad in ((1, 4, 10), (0, 4, 9), (0, 0, 10), (0, 10, 10), (0, 11, 10)):
        assert evidence(bounds=(ctypes.c_int64 * 3)(*bad)) == EINVAL, bad
        assert b"bounds" in L.qn_last_error()

    def tune(**kw):
        a = dict(n=5, B=2, p=10, bounds=good, G=2, tol=1e-8, max_iter=10, s2_min=1e-12, s2_max=1e12, tau_min=1e-12, tau_max=1e12,
                 tune_noise=1, tune_prior=1, cov_scale=1.0, s2=ptr, Dinv=None, ws_bytes=need)
        a.update(kw)
        return L.qn_la_tune(ptr, ptr, ptr, a["n"], a["B"], a["p"], a["bounds"], a["G"], ptr, ptr, a["tol"], a["max_iter"], a["s2_min"],
                            a["s2_max"], a["tau_min"], a["tau_max"], a["tune_noise"], a["tune_prior"], a["cov_scale"], a["s2"], ptr,
                            ptr, ptr, a["Dinv"], None, ptr, a["ws_bytes"], None)
    for kw in (dict(n=0), dict(G=0), dict(tol=-1.0), dict(tol=float("nan")), dict(max_iter=-1), dict(max_iter=100001),
               dict(s2_min=0.0), dict(s2_min=2.0, s2_max=1.0), dict(s2_max=float("inf")), dict(tau_min=-1.0),
               dict(tau_max=float("nan")), dict(tune_noise=2), dict(tune_prior=-1), dict(cov_scale=0.0),
               dict(cov_scale=float("inf")), dict(s2=None), dict(bounds=None), dict(bounds=(ctypes.c_int64 * 3)(0, 10, 10))):
        assert tune(**kw) == EINVAL, kw
        assert b"qn_la_tune" in L.qn_last_error()
    assert tune(ws_bytes=0) == EWORKSPACE
