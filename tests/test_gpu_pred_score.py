"""GPU: qn_pred_score (csrc/qn_score.hip) against the numpy restatement `score_np` of tests/test_pred_score_cpu.py over
every tail of both kernels, the cases where they can go wrong, the invariants the Python layer relies on, and the surface
built on it (`scoring.pred_score`, `QUiNNBase.score`, `NN_Laplace.score_glm`, examples/ex_score.py).

Bars per entry, absolute, eps = 2^-53 (`score_bars`); each follows from the arithmetic, none from what the kernels give:
  lppd    32 eps (max_m |ll_mk| + M + 1).  Each ll carries about 3 eps |ll| (the residual, its square, the division by s^2);
          that becomes a relative error of exp(ll - max); the sum of M positive terms adds at most M eps relative (the
          rescalings of the running maximum included); the log turns the relative error into an absolute one.  32 leaves ~5x.
  p_waic  64 eps (max_m |ll_mk| sd_m(ll) + var_m(ll)).  d var = 2 sd d ll with d ll = 3 eps |ll|, plus the Welford
          recurrence's own few eps of var.
  pit     1e-14: a mean of M values in [0, 1], each erfc good to a few eps.
  crps    8 eps M (max_m |y - f_mk| + max_m s_mk).  Two nested sums, of length M at most each, over terms of that size:
          the chained sums lose at most M eps relative, and the total divided by 2 M^2 is of the terms' size.
  mean    8 eps M max |f|: a recurrence of M roundings of size eps |f|.
  var     the same, times max |f - mean|.
A float32 F is compared with the restatement of the same float32 values read as float64.

Largest observed error / bar per row over the parity sweep (MI355X; also in profiles/pred_score.txt):
lppd 0.118, p_waic 0.850, pit 0.044, crps 0.163, mean 0.080, var 0.182.
The p_waic maximum is one entry of M = 2, K = 1025, V, sigma = 0.05 (0.71 in f64, 0.85 in f32; all other cases <= 0.12):
with s^2 below 1 / (2 pi) the log term of ll is negative and cancels the quadratic term there, |ll| = 0.01 beside terms of
0.5, and the bar is proportional to max |ll|.  The kernel therefore carries the roundings of the residual, its square, the
quotient and the sum along (`log_lik`, csrc/qn_score.hip); what is left is the error of log() itself, eps |log s^2|.  With
ll in plain float64 arithmetic that entry stood at 1.029 x the bar."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from quinn_amd import _lib, scoring
from test_pred_score_cpu import score_bars, score_np

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = scoring.WHAT_ALL
MS, KS, KMAX = (2, 3, 65, 257), (1, 63, 257, 1025), 1025
WORST = np.zeros(6)


def dev_rows(F, V, y, sigma, what=ALL):
    Ft = torch.as_tensor(np.ascontiguousarray(F)).cuda()
    Vt = None if V is None else torch.as_tensor(np.ascontiguousarray(V)).cuda()
    return scoring.score_rows(Ft, torch.as_tensor(np.asarray(y, dtype=np.float64)).cuda(), sigma, Vt, what).cpu().numpy()


def assert_within(got, ref, bars, rows=range(6), what=""):
    for r in rows:
        assert np.array_equal(np.isnan(got[r]), np.isnan(ref[r])), (what, r)
        ok = ~np.isnan(ref[r])
        ratio = np.abs(got[r][ok] - ref[r][ok]) / np.where(bars[r][ok] > 0, bars[r][ok], 1.0)
        exact = np.all(got[r][ok][bars[r][ok] == 0] == ref[r][ok][bars[r][ok] == 0])
        worst = float(ratio[bars[r][ok] > 0].max()) if np.any(bars[r][ok] > 0) else 0.0
        WORST[r] = max(WORST[r], worst)
        print(f"{what} row {scoring.ROWS[r]}: max error / bar = {worst:.3f}")
        assert exact and worst <= 1.0, (what, scoring.ROWS[r], worst)


def _data(M, dtype, seed=0):
    rs = np.random.RandomState(1000 * M + seed)
    mu = rs.randn(KMAX) * 2.0
    F = (mu + 0.5 * rs.randn(M, KMAX)).astype(dtype)
    V = rs.uniform(0.01, 0.5, size=(M, KMAX)).astype(dtype)
    y = mu + 0.7 * rs.randn(KMAX)
    return F, V, y


_REF = {}


def _reference(M, dtype, with_v, sigma):
    """(F, V, y, reference rows, bars) at K = KMAX, computed once per combination: an entry's numbers do not depend on K,
    so the smaller K take the first columns."""
    key = (M, np.dtype(dtype).name, with_v, sigma)
    if key not in _REF:
        F, V, y = _data(M, dtype)
        V = V if with_v else None
        _REF[key] = (F, V, y, score_np(F, V, y, sigma), score_bars(F, V, y, sigma))
    return _REF[key]


@pytest.mark.parametrize("sigma", [0.05, 1.0])
@pytest.mark.parametrize("with_v", [False, True], ids=["noV", "V"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("M", MS)
def test_kernel_equals_numpy(M, K, dtype, with_v, sigma):
    F, V, y, ref, bars = _reference(M, dtype, with_v, sigma)
    got = dev_rows(F[:, :K], None if V is None else V[:, :K], y[:K], sigma)
    assert_within(got, ref[:, :K], bars[:, :K], what=f"M={M} K={K}")
    print("largest error / bar so far, rows", scoring.ROWS, ":", " ".join(f"{w:.3f}" for w in WORST))


# ------------------------------------------------------------------------------------------ where the kernels can go wrong
def test_far_member_keeps_lppd_finite():
    rs = np.random.RandomState(1)
    M, K, s = 9, 70, 0.5
    y = rs.randn(K)
    F = y + s * rs.randn(M, K)
    for far in (0, 4, M - 1):                                # first (the running maximum starts there), middle, last
        G = F.copy()
        G[far] = y + 1e4 * s                                 # z = 1e4: ll about -5e7
        got = dev_rows(G, None, y, s)
        assert np.isfinite(got).all()
        assert_within(got, score_np(G, None, y, s), score_bars(G, None, y, s), what=f"far member {far}")


def test_large_common_offset_keeps_p_waic():
    rs = np.random.RandomState(2)
    M, K, s = 33, 70, 1.0
    y = rs.randn(K)
    F = y + 3e3 + rs.randn(M, K)                             # ll near -4.5e6, spread of z about 1
    got = dev_rows(F, None, y, s)
    ref = score_np(F, None, y, s)
    assert np.all(ref[0] < -4e6) and np.all(ref[1] > 1e5)
    assert_within(got, ref, score_bars(F, None, y, s), what="offset")


def test_identical_members_are_exact():
    rs = np.random.RandomState(3)
    M, K = 37, 130
    f, y = rs.randn(K) * 10, rs.randn(K) * 10
    F = np.tile(f, (M, 1))
    got = dev_rows(F, None, y, 0.3)
    assert np.all(got[1] == 0.0) and np.all(got[5] == 0.0) and np.array_equal(got[4], f)
    got0 = dev_rows(F, None, y, 0.0, _lib.SCORE_CRPS | _lib.SCORE_MOMENTS)
    assert np.array_equal(got0[3], np.abs(y - f)) and np.all(got0[5] == 0.0)


@pytest.mark.parametrize("M,K", [(3, 63), (65, 257), (257, 65)])
def test_sigma_zero_is_the_ensemble_crps(M, K):
    F, _, y = _data(M, np.float64, seed=5)
    F, y = F[:, :K], y[:K]
    what = _lib.SCORE_CRPS | _lib.SCORE_MOMENTS
    got = dev_rows(F, None, y, 0.0, what)
    ref = score_np(F, None, y, 0.0)
    assert np.isnan(got[:3]).all()                           # not asked for: the NaN the buffer was filled with
    assert_within(got, ref, score_bars(F, None, y, 0.0), rows=(3, 4, 5), what=f"sigma=0 M={M}")


def test_pit_keeps_relative_accuracy_in_the_tail():
    M, K, s = 4, 64, 0.25
    f = np.linspace(-1, 1, K)
    F = np.tile(f, (M, 1)) + np.arange(M)[:, None] * 1e-3
    y = f - 9 * s                                            # z = -9 and a little below: pit about 1e-19
    got = dev_rows(F, None, y, s, _lib.SCORE_PIT)[2]
    ref = score_np(F, None, y, s, crps=False)[2]
    assert np.all(ref < 2e-19) and np.all(ref > 0)
    assert np.max(np.abs(got / ref - 1)) <= 1e-10


def test_zero_member_variance():
    F, V, y = _data(5, np.float64, seed=6)
    F, V, y = F[:, :70].copy(), V[:, :70].copy(), y[:70]
    V[2, 11] = 0.0
    F[2, 12], V[2, 12] = y[12], 0.0                          # f == y exactly at s = 0: the member counts 0.5
    got = dev_rows(F, V, y, 0.0)
    ref = score_np(F, V, y, 0.0)
    assert np.isnan(got[:2, 11:13]).all() and np.isfinite(got[2:, 11:13]).all()
    assert_within(got, ref, score_bars(F, V, y, 0.0), rows=(2, 3, 4, 5), what="s=0")
    keep = np.ones(70, dtype=bool)
    keep[11:13] = False
    assert_within(got[:, keep], ref[:, keep], score_bars(F, V, y, 0.0)[:, keep], what="s=0, others")


def test_bad_values_poison_their_entry_only():
    F, V, y = _data(65, np.float64, seed=7)
    F, V, y = F[:, :257].copy(), V[:, :257].copy(), y[:257]
    clean = dev_rows(F, V, y, 0.1)
    assert np.isfinite(clean).all()
    F[64, 3], F[0, 100], V[33, 256] = np.nan, np.inf, -1.0
    got = dev_rows(F, V, y, 0.1)
    bad = np.zeros(257, dtype=bool)
    bad[[3, 100, 256]] = True
    assert np.isnan(got[:, bad]).all()
    assert np.array_equal(got[:, ~bad], clean[:, ~bad])
    y2 = y.copy()
    y2[7] = np.nan
    got = dev_rows(F, V, y2, 0.1)
    bad[7] = True
    assert np.isnan(got[:, bad]).all() and np.array_equal(got[:, ~bad], clean[:, ~bad])


# ------------------------------------------------------------------------------------------ invariants
@pytest.mark.parametrize("with_v", [False, True], ids=["noV", "V"])
def test_bits_repeat_and_do_not_depend_on_the_other_entries(with_v):
    F, V, y = _data(65, np.float32 if with_v else np.float64, seed=8)
    V = V if with_v else None
    one = dev_rows(F, V, y, 0.3)
    assert np.array_equal(one, dev_rows(F, V, y, 0.3))
    a = dev_rows(F[:, :257], None if V is None else V[:, :257], y[:257], 0.3)
    b = dev_rows(F[:, 257:], None if V is None else V[:, 257:], y[257:], 0.3)
    assert np.array_equal(np.concatenate([a, b], axis=1), one)


def test_what_subsets_leave_other_rows_untouched():
    F, V, y = _data(3, np.float64, seed=9)
    full = dev_rows(F, V, y, 0.3)
    bits = (_lib.SCORE_LPPD, _lib.SCORE_PWAIC, _lib.SCORE_PIT, _lib.SCORE_CRPS, _lib.SCORE_MOMENTS)
    rows_of = ((0,), (1,), (2,), (3,), (4, 5))
    for what in (1, 2, 4, 8, 16, 1 | 4, 2 | 8 | 16):
        got = dev_rows(F, V, y, 0.3, what)                   # score_rows fills the buffer with NaN before the call
        asked = [r for b, rs_ in zip(bits, rows_of) if what & b for r in rs_]
        for r in range(6):
            if r in asked:
                assert np.array_equal(got[r], full[r]), (what, r)
            else:
                assert np.isnan(got[r]).all(), (what, r)


def test_workspace_one_byte_short():
    L = _lib.lib()
    M, K = 33, 100
    need = L.qn_pred_score_workspace_bytes(M, K, ALL)
    F = torch.zeros(M, K, dtype=torch.float64, device="cuda")
    y = torch.zeros(K, dtype=torch.float64, device="cuda")
    out = torch.full((6, K), 7.0, dtype=torch.float64, device="cuda")
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    rc = L.qn_pred_score(F.data_ptr(), None, 0, y.data_ptr(), M, K, 1.0, ALL, out.data_ptr(), ws.data_ptr(), need - 1, None)
    assert rc == -2 and b"workspace" in L.qn_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


# ------------------------------------------------------------------------------------------ surface
PER_ENTRY = scoring.ROWS


def _problem(N, seed=0):
    rs = np.random.RandomState(seed)
    x = rs.rand(N, 1) * 6 - 3
    return x, np.sin(x) + 0.1 * rs.randn(N, 1)


@pytest.fixture(scope="module")
def ens():
    from quinn_amd.nns.mlp import MLP
    from quinn_amd.solvers.nn_ens import NN_Ens
    torch.manual_seed(0)
    np.random.seed(0)
    x, y = _problem(64)
    uq = NN_Ens(MLP(1, 1, (16, 16), activ='tanh').double(), nens=8, dfrac=0.8, verbose=False)
    uq.fit(x, y, lrate=0.01, batch_size=16, nepochs=5, freq_out=1000)
    return uq


def test_solver_score_equals_pred_score_on_predict_ens(ens):
    xt, yt = _problem(37, seed=1)
    np.random.seed(5)
    s = ens.score(xt, yt, noise=0.1)
    np.random.seed(5)                                        # the same permutation of the members
    r = scoring.pred_score(ens.predict_ens(xt), yt, 0.1)
    for k in PER_ENTRY:
        assert s[k].shape == yt.shape and np.array_equal(s[k], r[k]), k
    for k in ("lppd", "p_waic", "elpd_waic", "waic", "se_elpd", "nlpd", "crps", "rmse"):
        assert s[k] == r[k] and np.isfinite(s[k]), k
    assert s["coverage"] == r["coverage"] and set(s["coverage"]) == {0.5, 0.9, 0.95}
    assert s["pit_hist"].sum() == 37
    np.random.seed(5)
    c = ens.score(xt, yt, noise=0.1, max_bytes=8 * 1 * 8 * 5)      # 8 members x 1 output x 8 bytes: 5 rows per chunk
    for k in PER_ENTRY:
        assert np.array_equal(c[k], s[k]), k
    with pytest.raises(ValueError):
        ens.score(xt, yt)                                    # NN_Ens keeps no data noise
    nc = ens.score(xt, yt, noise=0.1, crps=False)
    assert np.isnan(nc["crps_k"]).all() and np.isnan(nc["crps"]) and np.isfinite(nc["lppd"])


def test_mcmc_score_pools_chains():
    from quinn_amd.nns.mlp import MLP
    from quinn_amd.solvers.nn_mcmc import NN_MCMC
    x, y = _problem(48)
    xt, yt = _problem(37, seed=1)
    torch.manual_seed(0)
    uq = NN_MCMC(MLP(1, 1, (8, 8), activ='tanh'), verbose=False)
    ini = np.stack([np.random.RandomState(100 + c).rand(uq.pdim) * 0.2 for c in range(4)])
    uq.fit(x, y, zflag=False, datanoise=0.2, nmcmc=60, param_ini=ini, sampler='hmc',
           sampler_params={'epsilon': 1e-3, 'L': 3}, nchains=4, seeds=list(range(4)), engine='device')
    s = uq.score(xt, yt, nsam=20, nburn=20, chain='all')     # noise: the fit's datanoise
    F = uq.predict_ens(xt, nens=20, nburn=20, chain='all')
    assert F.shape[0] == 20
    ref = score_np(F.reshape(20, -1), None, yt.reshape(-1), 0.2)
    bars = score_bars(F.reshape(20, -1), None, yt.reshape(-1), 0.2)
    assert np.all(np.abs(s["lppd_k"].reshape(-1) - ref[0]) <= bars[0])
    assert abs(s["lppd"] - ref[0].sum()) <= bars[0].sum()


def test_laplace_score_glm_and_predict_glm_unchanged():
    from quinn_amd.nns.mlp import MLP
    from quinn_amd.ops import BatchedMLP
    from quinn_amd.solvers import NN_Laplace
    from quinn_amd.solvers.nn_laplace import glm_mixture
    torch.manual_seed(0)
    np.random.seed(0)
    x, y = _problem(40)
    xt, yt = _problem(37, seed=1)
    la = NN_Laplace(MLP(1, 1, (11, 11), biasorno=True, activ='tanh').double(), la_type='ggn_diag', nens=3, dfrac=0.8,
                    datanoise=0.1, verbose=False)
    la.fit(x, y, val=[xt, yt], lrate=0.01, batch_size=8, nepochs=30, freq_out=1000)
    op = BatchedMLP(la.arch, xt, None, device=la._device)
    f, S = op.glm_predict(np.asarray(la.means), torch.stack([c for c in la._cov_dev]))
    f, S = f.cpu().numpy(), S.cpu().numpy()
    s = la.score_glm(xt, yt)
    F, V = f.reshape(3, -1), S[:, :, 0, 0].reshape(3, -1)
    ref, bars = score_np(F, V, yt.reshape(-1), 0.1), score_bars(F, V, yt.reshape(-1), 0.1)
    got = np.stack([s[k].reshape(-1) for k in PER_ENTRY])
    assert_within(got, ref, bars, what="score_glm")
    assert np.isfinite(s["waic"]) and s["n"] == 37
    mean, cov = glm_mixture(f, S)                            # predict_glm: bit for bit what it was before the helper
    ym, yv, yc = la.predict_glm(xt, msc=2)
    assert np.array_equal(ym, mean) and np.array_equal(yc, cov) and np.array_equal(yv[:, 0], cov[:, 0, 0])


def test_example_runs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "ex_score.py")], cwd=ROOT, capture_output=True,
                       text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "nlpd" in r.stdout and "score_glm" in r.stdout
