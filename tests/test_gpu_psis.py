"""GPU: qn_psis_loo (csrc/qn_psis.hip) against its authority `psis.psis_loo_rows` run in np.longdouble on the same
(float32-rounded, where applicable) inputs, over every tail of the three kernels -- M below and above the smoothing limit of
21, one member-chunk of 512, one chunk plus 1 and two chunks plus 1, every M with float64 and float32 F, with and without V and at
both sigma; K below, at and above the tile of 4 and the wave of 64 --
its determinism, ties on the cutoff, the isolation of bad entries, every refusal, and the surface built on it
(`scoring.pred_score`, `QUiNNBase.score`, `NN_Laplace.score_glm` with loo=True).

Bounds (BOUND): 4 x the largest deviation measured on the MI355X over the parity sweep and the ties test, per row; khat,
elpd_loo_k and pit_loo absolute, ess_k relative to M.  The device's exp / log1p / erfc differ from libm by a few ulp and the
profile likelihood sums m T <= 2e4 of them; a deviation above 1e-9 would mean a branch (tail membership, the x_q <= 0 rule)
decided differently.  Measured maxima over the sweep (MI355X): elpd_loo_k 1.092e-12, khat 6.915e-12 (an entry of the heavy
rows, whose khat is of order 10), ess_k / M 4.025e-13, pit_loo 2.110e-15; the ties test stays below 4e-15 in every row.
Bounds: elpd_loo_k 4.4e-12, khat 2.8e-11, ess_k / M 1.6e-12, pit_loo 8.4e-15."""
import numpy as np
import pytest
import torch

from quinn_amd import _lib, psis, scoring
from test_psis_cpu import HEAVY, KMAX, LD, loo_reference

pytestmark = pytest.mark.gpu

CHUNK = 512                                                 # PCH of csrc/qn_psis.hip
MS = (2, 20, 21, 24, 25, 64, 257, 1000, CHUNK + 1, 2 * CHUNK + 1)
KS = (1, 63, 65, 257)
VARIANTS = [(d, v, s) for d in (np.float64, np.float32) for v in (False, True) for s in (0.05, 1.0)]
MEASURED = {"elpd_loo_k": 1.092e-12, "khat": 6.915e-12, "ess_k": 4.025e-13, "pit_loo": 2.110e-15}       # MI355X, this file's sweep
BOUND = {k: 4.0 * v for k, v in MEASURED.items()}
WORST = np.zeros(4)


def dev_rows(F, V, y, sigma):
    Ft = torch.as_tensor(np.ascontiguousarray(F)).cuda()
    Vt = None if V is None else torch.as_tensor(np.ascontiguousarray(V)).cuda()
    return scoring.psis_rows(Ft, torch.as_tensor(np.asarray(y, dtype=np.float64)).cuda(), sigma, Vt).cpu().numpy()


def assert_within(got, ref, M, what=""):
    """Deviation of the device rows from the longdouble rows `ref`, row by row, against BOUND; NaN and Inf must coincide."""
    ref64 = ref.astype(np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(ref64)), what
    assert np.array_equal(np.isinf(got), np.isinf(ref64)) and np.array_equal(got[np.isinf(got)], ref64[np.isinf(got)]), what
    for r, name in enumerate(psis.ROWS):
        ok = np.isfinite(got[r])
        dev = float(np.max(np.abs(got[r][ok].astype(LD) - ref[r][ok]), initial=0.0)) / (M if name == "ess_k" else 1)
        WORST[r] = max(WORST[r], dev)
        print(f"{what} row {name}: max deviation {dev:.3e}")
        assert dev <= BOUND[name], (what, name, dev)


def _cases():
    for M in MS:
        for dtype, with_v, sigma in VARIANTS:
            yield pytest.param(M, dtype, with_v, sigma, id=f"M{M}-{np.dtype(dtype).name}-{'V' if with_v else 'noV'}-{sigma}")


@pytest.mark.parametrize("M,dtype,with_v,sigma", list(_cases()))
def test_kernel_equals_authority(M, dtype, with_v, sigma):
    F, V, y, ref = loo_reference(M, dtype, sigma, with_v)
    for K in KS:
        got = dev_rows(F[:, :K], None if V is None else V[:, :K], y[:K], sigma)
        assert_within(got, ref[:, :K], M, what=f"M={M} K={K}")
    if M >= 64:
        assert np.median(got[1, HEAVY]) > 0.7                 # the targets 6 standard deviations out are flagged
    if M < 21:
        assert np.all(np.isposinf(got[1]))
    print("largest deviation so far, rows", psis.ROWS, ":", " ".join(f"{w:.3e}" for w in WORST))


# ------------------------------------------------------------------------------------------ determinism
def test_two_calls_and_single_column_give_the_same_bits():
    for M, dtype, with_v in ((2 * CHUNK + 1, np.float32, True), (64, np.float64, False), (20, np.float64, True)):
        F, V, y, _ = loo_reference(M, dtype, 1.0, with_v)
        a = dev_rows(F, V, y, 1.0)
        assert np.array_equal(a, dev_rows(F, V, y, 1.0), equal_nan=True)
        for k in (0, 3, 130, KMAX - 1):
            one = dev_rows(F[:, k:k + 1], None if V is None else V[:, k:k + 1], y[k:k + 1], 1.0)
            assert np.array_equal(one[:, 0], a[:, k]), (M, k)


# ------------------------------------------------------------------------------------------ ties
def test_ties_on_the_cutoff():
    """Float32 members in exact copies: M = 90 members are 30 distinct ones three times (T = 18: the cutoff falls inside a
    triple, and q = 5 with x_q > 0), and M = 64 members are 2 distinct ones (every excess is 0: no smoothing).  The tail is the
    one of the (lr, m) order, so the rows equal the authority's within the parity bound."""
    rs = np.random.RandomState(7)
    K = 70
    y = rs.randn(K)
    base = (y + 0.5 * rs.randn(30, K)).astype(np.float32)
    F = np.concatenate([base, base, base])[rs.permutation(90)]
    ref = psis.psis_loo_rows(F, y, 0.6, dtype=LD)
    got = dev_rows(F, None, y, 0.6)
    assert np.isfinite(ref[1].astype(np.float64)).all()
    assert_within(got, ref, 90, what="triples")
    F = np.concatenate([np.tile(base[:1], (40, 1)), np.tile(base[1:2], (24, 1))])[rs.permutation(64)]
    ref = psis.psis_loo_rows(F, y, 0.6, dtype=LD)
    got = dev_rows(F, None, y, 0.6)
    assert np.all(np.isposinf(got[1]))
    assert_within(got, ref, 64, what="two values")


# ------------------------------------------------------------------------------------------ isolation
def test_bad_entries_stay_alone():
    for dtype in (np.float64, np.float32):
        F, V, y, _ = loo_reference(CHUNK + 1, dtype, 0.05, True)
        F, V, y = F[:, :70].copy(), V[:, :70].copy(), y[:70].copy()
        clean = dev_rows(F, V, y, 0.05)
        assert np.isfinite(clean[[0, 2, 3]]).all()
        F[300, 5], y[6], V[CHUNK, 64], V[0, 69] = np.nan, np.inf, -1.0, np.inf
        got = dev_rows(F, V, y, 0.05)
        bad = np.zeros(70, dtype=bool)
        bad[[5, 6, 64, 69]] = True
        assert np.isnan(got[:, bad]).all()
        assert np.array_equal(got[:, ~bad], clean[:, ~bad])


# ------------------------------------------------------------------------------------------ refusals
def test_refusals_touch_nothing():
    L = _lib.lib()
    M, K = 33, 100
    need = L.qn_psis_loo_workspace_bytes(M, K)
    F = torch.zeros(M, K, dtype=torch.float64, device="cuda")
    y = torch.zeros(K, dtype=torch.float64, device="cuda")
    out = torch.full((4, K), 7.0, dtype=torch.float64, device="cuda")
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")

    def call(F=F.data_ptr(), V=None, dtype=0, Y=y.data_ptr(), M=M, K=K, sigma=1.0, out=out.data_ptr(), ws=ws.data_ptr(), nbytes=need):
        return L.qn_psis_loo(F, V, dtype, Y, M, K, sigma, out, ws, nbytes, None)

    for kw in ({"M": 1}, {"M": _lib.PSIS_MAX_M + 1}, {"K": 0}, {"K": 2 ** 31 + 1}, {"dtype": 2}, {"sigma": -1.0}, {"sigma": float("nan")},
               {"sigma": float("inf")}, {"sigma": 0.0}, {"F": None}, {"Y": None}, {"out": None}, {"ws": None}):
        assert call(**kw) == -1 and L.qn_last_error(), kw
    assert call(nbytes=need - 1) == -2 and b"workspace" in L.qn_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((out[1] == float("inf")).all())              # identical members: no smoothing


# ------------------------------------------------------------------------------------------ solvers
PARENT_KEYS = set(scoring.ROWS) | {"n", "lppd", "p_waic", "elpd_waic", "waic", "se_elpd", "nlpd", "crps", "rmse", "coverage",
                                   "pit_hist"}
LOO_KEYS = set(psis.ROWS) | {"elpd_loo", "looic", "se_elpd_loo", "khat_threshold", "n_khat_bad", "khat_bad", "coverage_loo",
                             "pit_loo_hist", "p_loo"}


def _problem(N, seed=0):
    rs = np.random.RandomState(seed)
    x = rs.rand(N, 1) * 6 - 3
    return x, np.sin(x) + 0.1 * rs.randn(N, 1)


def _mcmc(**fit_args):
    from quinn_amd.nns.mlp import MLP
    from quinn_amd.solvers.nn_mcmc import NN_MCMC
    x, y = _problem(40)
    torch.manual_seed(0)
    uq = NN_MCMC(MLP(1, 1, (8, 8), activ='tanh'), verbose=False)
    ini = np.stack([np.random.RandomState(100 + c).rand(uq.pdim) * 0.2 for c in range(4)])
    uq.fit(x, y, zflag=False, datanoise=0.2, nmcmc=200, param_ini=ini, sampler='hmc', sampler_params={'epsilon': 1e-3, 'L': 3},
           nchains=4, seeds=list(range(4)), engine='device', **fit_args)
    return uq, x, y


def _check_solver(uq, x, y, **ens_args):
    s = uq.score(x, y, nsam=64, loo=True, **ens_args)
    assert set(s) == PARENT_KEYS | LOO_KEYS
    assert set(uq.score(x, y, nsam=64, **ens_args)) == PARENT_KEYS
    assert s["elpd_loo_k"].shape == y.shape and np.isfinite(s["elpd_loo_k"]).all()
    assert s["elpd_loo"] <= s["lppd"] and s["p_loo"] == s["lppd"] - s["elpd_loo"]
    assert s["khat_threshold"] == psis.khat_threshold(64)
    M, o = 64, y.shape[1]
    esize = 4 if uq._dtype == "float32" else 8
    c = uq.score(x, y, nsam=64, loo=True, max_bytes=M * o * esize * 14, **ens_args)          # 14 rows per chunk: 3 chunks of 40
    for k in psis.ROWS:
        assert np.array_equal(c[k], s[k]), k
    return s


def test_mcmc_score_loo():
    uq, x, y = _mcmc()
    s = _check_solver(uq, x, y, nburn=100, chain='all')
    r = scoring.pred_score(uq.predict_ens(x, nens=64, nburn=100, chain='all'), y, 0.2, loo=True)
    assert set(r) == PARENT_KEYS | LOO_KEYS
    for k in psis.ROWS:
        assert np.array_equal(r[k], s[k]), k


def test_mcmc_noiseprior_score_loo_goes_through_v():
    uq, x, y = _mcmc(noiseprior=dict(a0=3.0, b0=0.1))
    assert uq._score_member_noise(None, 64, nburn=100, chain='all') is not None
    _check_solver(uq, x, y, nburn=100, chain='all')


def test_laplace_score_glm_loo():
    from quinn_amd.nns.mlp import MLP
    from quinn_amd.solvers import NN_Laplace
    torch.manual_seed(0)
    np.random.seed(0)
    x, y = _problem(40)
    la = NN_Laplace(MLP(1, 1, (11, 11), biasorno=True, activ='tanh').double(), la_type='ggn', nens=24, dfrac=0.8,
                    datanoise=0.1, verbose=False)
    la.fit(x, y, val=[x, y], lrate=0.01, batch_size=8, nepochs=10, freq_out=1000)
    s = la.score_glm(x, y, loo=True)
    assert set(s) == PARENT_KEYS | LOO_KEYS and set(la.score_glm(x, y)) == PARENT_KEYS
    assert np.isfinite(s["khat"]).any() and s["khat_threshold"] == psis.khat_threshold(24)     # 24 members: T = 5, smoothed
    assert np.isfinite(s["elpd_loo_k"]).all() and s["elpd_loo"] <= s["lppd"]
    f, S = la._glm_members(x)                                  # the same F and V through the front end of any ensemble
    V = torch.diagonal(S, dim1=-2, dim2=-1).contiguous()
    r = scoring.pred_score(f, y, 0.1, V=V, loo=True)
    for k in psis.ROWS:
        assert np.array_equal(r[k], s[k], equal_nan=True), k
