"""GPU: qn_stack_weights, qn_group_lpd and qn_pred_score_w (csrc/qn_stack.hip) against their contract
`quinn_amd/stacking.py`, and the surface built on them (`scoring.group_lpd` / `stack_weights` / `pred_score`,
`QUiNNBase.score(member_weights=)`, `NN_MCMC.stack`, `NN_Ens.stack`, `predict_mom_stacked`).  Every randomised input comes
from tests/test_stacking_cpu.py, which checks that the contract stops on it by its gap within a quarter of the iteration cap.

Bars.  qn_stack_weights: w 1e-10 absolute and obj 1e-10 relative (the bars of tests/test_gpu_mlp_parity.py), iters and the
counts equal.  qn_group_lpd: 1e-13 against row 0 of qn_pred_score on the slice, and `score_bars` row 0 (32 eps (max |ll| +
M_g + 1), tests/test_gpu_pred_score.py) against the contract in np.longdouble.  qn_pred_score_w at wm = 1 / M: 1e-12 of the
row's largest magnitude against qn_pred_score; at random weights the per-entry bars of `score_bars` against the contract in
np.longdouble -- weights in [0, 1] that sum to 1 make no term of any sum larger than in the equal-weight derivation -- with
pit held to the 8.4e-15 of tests/test_gpu_psis.py."""
import numpy as np
import pytest
import torch

from quinn_amd import _lib, scoring, stacking
from test_pred_score_cpu import score_bars
from test_stacking_cpu import (DISJOINT_SIZES, LD, MAX_ITER, STACK_SHAPES, TOL, disjoint_L, lpd_data, slow_L, special_L, stack_L,
                               weights_data)

pytestmark = pytest.mark.gpu


def cuda(a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).cuda()


def dev_stack(L, block=64, tol=TOL, max_iter=MAX_ITER):
    return scoring.stack_weights(cuda(np.asarray(L, dtype=np.float64)), tol=tol, max_iter=max_iter, block=block)


def assert_stack_parity(got, ref, what=""):
    dw = float(np.max(np.abs(got["w"] - ref["w"])))
    dobj = abs(got["obj"] - ref["obj"]) / max(abs(ref["obj"]), 1e-300)
    print(f"{what}: iters {got['iters']} (contract {ref['iters']}) max |dw| {dw:.2e} rel dobj {dobj:.2e} gap {got['gap']:.3e}")
    assert got["iters"] == ref["iters"], what
    assert (got["n_kept"], got["n_dropped"], got["n_nonfinite"]) == (ref["n_kept"], ref["n_dropped"], ref["n_nonfinite"]), what
    assert dw <= 1e-10 and dobj <= 1e-10, what
    assert abs(got["obj_equal"] - ref["obj_equal"]) <= 1e-10 * abs(ref["obj_equal"]) and abs(got["gap"] - ref["gap"]) <= 1e-8, what


# ------------------------------------------------------------------------------------------ qn_stack_weights
@pytest.mark.parametrize("G,K", STACK_SHAPES)
def test_stack_weights_equal_contract(G, K):
    L = stack_L(G, K)
    got = dev_stack(L)
    assert_stack_parity(got, stacking.stack_weights(L, TOL, MAX_ITER), f"G={G} K={K}")
    assert got["gap"] <= TOL and abs(got["w"].sum() - 1) < 1e-12


def test_stack_weights_bits_do_not_depend_on_block_or_call():
    L = slow_L()                                               # hundreds of iterations: several blocks of 64 launches
    ref = stacking.stack_weights(L, TOL, MAX_ITER)
    assert ref["iters"] > 128
    assert_stack_parity(dev_stack(L), ref, "slow")
    for L in (L, stack_L(65, 1000)):
        a, b, c = dev_stack(L, block=64), dev_stack(L, block=1), dev_stack(L, block=64)
        for other in (b, c):
            assert np.array_equal(a["w"], other["w"]) and all(a[k] == other[k] for k in a if k != "w")


def test_stack_weights_disjoint_support():
    got = dev_stack(disjoint_L())
    assert got["iters"] == 1
    assert np.max(np.abs(got["w"] - np.array(DISJOINT_SIZES) / np.sum(DISJOINT_SIZES))) <= 1e-15


def test_stack_weights_nonfinite_and_dropped_entries():
    L = special_L()
    got = dev_stack(L)
    assert (got["n_dropped"], got["n_nonfinite"], got["n_kept"]) == (3, 7, 254)
    assert_stack_parity(got, stacking.stack_weights(L, TOL, MAX_ITER), "special")
    e = dev_stack(np.full((3, 4), -np.inf))
    assert e["n_kept"] == 0 and np.all(e["w"] == 1 / 3) and e["obj"] == 0 and e["iters"] == 0
    capped = dev_stack(stack_L(5, 257), max_iter=3)
    assert capped["iters"] == 3 and capped["gap"] > TOL
    assert_stack_parity(capped, stacking.stack_weights(stack_L(5, 257), TOL, 3), "max_iter = 3")


def test_stack_weights_many_tiles():
    """K = 256 * 256 + 300: more tiles than blocks, so a block owns two tiles and the last tile is partial."""
    K = 256 * 256 + 300
    L = np.tile(stack_L(3, 1000), (1, K // 1000 + 1))[:, :K]
    assert_stack_parity(dev_stack(L), stacking.stack_weights(L, TOL, MAX_ITER), f"G=3 K={K}")


# ------------------------------------------------------------------------------------------ qn_group_lpd
UNEVEN = np.array([0, 2, 3, 40, 64, 65, 129, 130])


@pytest.mark.parametrize("with_v", [False, True], ids=["noV", "V"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("M,K,offsets", [(7, 65, np.array([0, 1, 3, 7])), (130, 129, UNEVEN)], ids=["7x65", "130x129"])
def test_group_lpd(M, K, offsets, dtype, with_v):
    F, V, y = lpd_data(M, K, dtype, with_v)
    sigma = 0.3
    Ft, Vt, yt = cuda(F), cuda(V), cuda(y)
    got = scoring.group_lpd_rows(Ft, yt, sigma, offsets, Vt).cpu().numpy()
    ref = stacking.group_lpd(F, y, sigma, offsets, V, dtype=LD)
    assert np.array_equal(got, scoring.group_lpd(Ft, yt, sigma, offsets, Vt)[0].cpu().numpy())
    for g in range(len(offsets) - 1):
        lo, hi = offsets[g], offsets[g + 1]
        Vg = None if V is None else V[lo:hi]
        bar = score_bars(np.concatenate([F[lo:hi]] * 2), None if V is None else np.concatenate([Vg] * 2), y, sigma)[0] \
            if hi - lo == 1 else score_bars(F[lo:hi], Vg, y, sigma)[0]
        dev = np.abs(got[g].astype(LD) - ref[g]).astype(np.float64)
        print(f"group {g} of {hi - lo}: max deviation / bar {np.max(dev / bar):.3f}")
        assert np.all(dev <= bar), g
        if hi - lo >= 2:
            row0 = scoring.score_rows(Ft[lo:hi].contiguous(), yt, sigma, None if V is None else Vt[lo:hi].contiguous(),
                                      _lib.SCORE_LPPD).cpu().numpy()[0]
            assert np.max(np.abs(got[g] - row0)) <= 1e-13, g
    F2 = F.copy()
    F2[offsets[1], K // 2] = np.nan                            # the first member of group 1, one entry
    bad = scoring.group_lpd_rows(cuda(F2), yt, sigma, offsets, Vt).cpu().numpy()
    assert np.isnan(bad[1, K // 2]) and np.isnan(bad).sum() == 1
    bad[1, K // 2] = got[1, K // 2]
    assert np.array_equal(bad, got)


# ------------------------------------------------------------------------------------------ qn_pred_score_w
def dev_rows_w(F, V, y, sigma, wm, what=scoring.WHAT_ALL):
    return scoring.score_rows_w(cuda(F), cuda(None if y is None else np.asarray(y, dtype=np.float64)), sigma,
                                cuda(np.asarray(wm, dtype=np.float64)), cuda(V), what).cpu().numpy()


@pytest.mark.parametrize("K", [1, 129])
@pytest.mark.parametrize("M", [2, 33, 130])
def test_pred_score_w_at_equal_weights_is_pred_score(M, K):
    for dtype, with_v, sigma in ((np.float64, False, 0.3), (np.float32, True, 0.05)):
        F, V, y = lpd_data(M, K, dtype, with_v)
        got = dev_rows_w(F, V, y, sigma, np.full(M, 1.0 / M))
        ref = scoring.score_rows(cuda(F), cuda(y), sigma, cuda(V)).cpu().numpy()
        for r, name in enumerate(scoring.ROWS):
            rel = np.max(np.abs(got[r] - ref[r])) / np.max(np.abs(ref[r]))
            print(f"M={M} K={K} {np.dtype(dtype).name} row {name}: {rel:.2e} of the row's largest magnitude")
            assert rel <= 1e-12, name


@pytest.mark.parametrize("M", [5, 33, 130])
def test_pred_score_w_random_weights_equal_contract(M):
    for dtype, with_v, sigma in ((np.float64, True, 0.05), (np.float32, False, 0.3)):
        F, V, y = lpd_data(M, 129, dtype, with_v)
        wm = weights_data(M)
        got = dev_rows_w(F, V, y, sigma, wm)
        ref = stacking.weighted_rows(F, y, sigma, wm, V, dtype=LD)
        bars = score_bars(F, V, y, sigma)
        bars[2] = 8.4e-15
        for r, name in enumerate(scoring.ROWS):
            ratio = float(np.max(np.abs(got[r].astype(LD) - ref[r]).astype(np.float64) / bars[r]))
            print(f"M={M} {np.dtype(dtype).name} row {name}: max deviation / bar {ratio:.3f}")
            assert ratio <= 1.0, name
        assert np.array_equal(got, dev_rows_w(F, V, y, sigma, wm))
        one = dev_rows_w(F[:, 7:8], None if V is None else V[:, 7:8], y[7:8], sigma, wm)
        assert np.array_equal(one[:, 0], got[:, 7])


def test_pred_score_w_rules():
    M, K, sigma = 33, 70, 0.2
    F, V, y = lpd_data(M, K, np.float64, True)
    wm = weights_data(M)
    clean = dev_rows_w(F, V, y, sigma, wm)
    assert np.isfinite(clean).all()
    Fn, Vn = F.copy(), V.copy()
    Fn[wm == 0], Vn[wm == 0] = np.nan, np.inf                  # a zero-weight member is skipped entirely
    assert np.array_equal(dev_rows_w(Fn, Vn, y, sigma, wm), clean)
    hot = np.zeros(M)
    hot[32] = 1.0
    Fh = F.copy()
    Fh[:32] = np.nan
    one = dev_rows_w(Fh, V, y, sigma, hot)
    s2 = sigma ** 2 + V[32]
    closed = stacking._crps_a(y - F[32], s2, np.float64) - 0.5 * stacking._crps_a(0 * y, 2 * s2, np.float64)
    assert np.all(one[1] == 0) and np.all(one[5] == 0) and np.array_equal(one[4], F[32])
    assert np.max(np.abs(one[3] - closed)) <= 1e-14 and np.max(np.abs(one[0] - stacking.weighted_rows(F, y, sigma, hot, V)[0])) <= 1e-13
    mom = dev_rows_w(F, None, None, 0.0, wm, _lib.SCORE_MOMENTS)                     # Y = NULL
    assert np.isnan(mom[:4]).all() and np.array_equal(mom[4:], clean[4:])
    for badw in (-1e-3, np.nan, np.inf):
        w2 = wm.copy()
        w2[3] = badw
        assert np.isnan(dev_rows_w(F, V, y, sigma, w2)).all()
    m1 = dev_rows_w(F[:1], V[:1], y, sigma, [1.0])             # M = 1 is legal here
    assert np.isfinite(m1).all() and np.all(m1[5] == 0)
    r = scoring.pred_score(F, y, sigma, V=V, member_weights=wm)
    assert np.array_equal(r["lppd_k"], clean[0]) and r["lppd"] == float(clean[0].sum())
    with pytest.raises(ValueError):
        scoring.pred_score(F, y, sigma, V=V, member_weights=wm, loo=True)


# ------------------------------------------------------------------------------------------ end to end
def _problem(N, seed):
    rs = np.random.RandomState(seed)
    x = rs.rand(N, 1) * 6 - 3
    return x, np.sin(x) + 0.1 * rs.randn(N, 1)


def test_ens_stack_discards_the_untrained_member():
    from quinn_amd.nns.mlp import MLP
    from quinn_amd.solvers.nn_ens import NN_Ens
    torch.manual_seed(0)
    np.random.seed(0)
    (x, y), (xt, yt) = _problem(64, 0), _problem(48, 1)
    uq = NN_Ens(MLP(1, 1, (16, 16), activ='tanh').double(), nens=6, dfrac=0.8)
    uq.fit(x, y, lrate=0.01, batch_size=16, nepochs=300, freq_out=10000)
    uq._best_w = np.array(uq._best_w)
    uq._best_w[0] = 0.5 * np.random.RandomState(5).randn(uq._best_w.shape[1])        # member 0: back to a random initialisation
    st = uq.stack(xt, yt, noise=0.1)
    print("weights", st["weights"], "elpd_stack", st["elpd_stack"], "elpd_equal", st["elpd_equal"], "iters", st["iters"])
    assert st is uq.stacking and st["weights"].shape == (6,) and np.array_equal(st["weights"], st["member_weights"])
    assert st["weights"][0] < 1 / (10 * 6) and abs(st["weights"].sum() - 1) < 1e-12
    assert st["elpd_stack"] >= st["elpd_equal"] and st["gap"] <= TOL and st["khat_bad_share"] is None
    assert st["n_dropped"] == 0 and st["n_nonfinite"] == 0
    s = uq.score(xt, yt, noise=0.1, nsam=6, member_weights=st["member_weights"])
    assert abs(s["lppd"] - st["elpd_stack"]) <= 1e-10 * abs(st["elpd_stack"])
    mean, var = uq.predict_mom_stacked(xt)
    F = uq._predict_batch(uq._best_w, xt)
    wm = st["member_weights"][:, None, None]
    assert np.max(np.abs(mean - (wm * F).sum(axis=0))) < 1e-12
    assert np.max(np.abs(var - (wm * (F - mean) ** 2).sum(axis=0) / (1 - (wm ** 2).sum()))) < 1e-12
    with pytest.raises(ValueError):
        uq.stack(xt, yt, noise=0.1, loo=True)


def test_mcmc_stack_loo_and_weighted_score():
    from quinn_amd.nns.mlp import MLP
    from quinn_amd.solvers.nn_mcmc import NN_MCMC
    x, y = _problem(64, 0)
    torch.manual_seed(0)
    uq = NN_MCMC(MLP(1, 1, (16, 16), activ='tanh'), verbose=False)
    ini = np.stack([np.random.RandomState(100 + c).rand(uq.pdim) * 0.2 for c in range(4)])
    uq.fit(x, y, zflag=False, datanoise=0.2, nmcmc=300, param_ini=ini, sampler='hmc', sampler_params={'epsilon': 1e-3, 'L': 3},
           nchains=4, seeds=list(range(4)), engine='device')
    ens = dict(nsam=128, nburn=100)
    st = uq.stack(x, y, loo=True, **ens)
    print("weights", st["weights"], "elpd_stack", st["elpd_stack"], "elpd_equal", st["elpd_equal"], "khat", st["khat_bad_share"])
    assert st["weights"].shape == (4,) and st["member_weights"].shape == (128,) and st["khat_bad_share"].shape == (4,)
    assert abs(st["weights"].sum() - 1) <= 1e-12 and abs(st["member_weights"].sum() - 1) <= 1e-12
    assert st["elpd_stack"] >= st["elpd_equal"] and st["gap"] <= TOL
    F = uq.predict_ens(x, nens=128, nburn=100, chain='all')
    s = uq.score(x, y, chain='all', member_weights=st["member_weights"], **ens)
    ll = -0.5 * ((y[None] - F) / 0.2) ** 2 - 0.5 * np.log(2 * np.pi * 0.04)
    on = st["member_weights"] > 0
    a = ll[on] + np.log(st["member_weights"][on])[:, None, None]
    host = a.max(axis=0) + np.log(np.exp(a - a.max(axis=0)).sum(axis=0))
    assert np.max(np.abs(s["lppd_k"] - host)) <= 1e-11 and abs(s["lppd"] - host.sum()) <= 1e-10 * abs(host.sum())
    # the defaults add nothing: score() is what it was, qn_pred_score on the downloaded ensemble
    d, r = uq.score(x, y, chain='all', **ens), scoring.pred_score(F, y, 0.2)
    assert set(d) == set(r)
    for k in scoring.ROWS:
        assert np.array_equal(d[k], r[k]), k
    held = uq.stack(x, y, loo=False, **ens)                     # the same chains through qn_group_lpd
    assert held["khat_bad_share"] is None and abs(held["weights"].sum() - 1) <= 1e-12
    with pytest.raises(ValueError):
        uq.score(x, y, chain='all', member_weights=st["member_weights"], loo=True, **ens)
