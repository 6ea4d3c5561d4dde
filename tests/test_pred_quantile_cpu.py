"""CPU: the numpy contract of the predictive quantiles (`quinn_amd/predquant.py`, the authority of `qn_pred_quantile`) against
np.quantile, plain bisection and closed forms; the header and its binding; and the refusals of the C entry points that need no
device.  `quant_inputs` and the level sets build the inputs of tests/test_gpu_pred_quantile.py."""
import ctypes
import re

import numpy as np
import pytest
from scipy.special import erfc

from quinn_amd import _lib, scoring
from quinn_amd import predquant as pq

MS = (1, 2, 3, 21, 64, 65, 513, 1025)
EMP_LEVELS = {1: [0.5], 3: [0.05, 0.5, 0.95], 8: [0.0, 0.001, 0.05, 0.25, 0.5, 0.77, 0.95, 1.0]}
MIX_LEVELS = {1: [0.5], 3: [0.05, 0.5, 0.95], 8: [1e-12, 0.001, 0.05, 0.25, 0.5, 0.77, 0.95, 0.999]}


def quant_inputs(kind, M, K, seed=0):
    """(F [M, K], V [M, K], sigma) of one input kind.  'cont': members around 3 with spread 0.3; 'ties': the same rounded to one
    decimal (no signed zeros), so that most members are tied; 'bimodal': every second member moved up by 40, far more than any
    s, which puts the levels near the share of the lower mode into the gap; 'f32': 'cont' in float32.  V is uniform in
    (0.01, 0.5) and sigma 0.1: mixed member spreads."""
    rs = np.random.RandomState(10000 + 31 * M + 7 * K + seed)
    F = 3.0 + 0.3 * rs.randn(M, K)
    V = 0.01 + 0.49 * rs.rand(M, K)
    if kind == "ties":
        F = np.round(F, 1) + 0.0
    elif kind == "bimodal":
        F[1::2] += 40.0
    elif kind == "f32":
        F, V = F.astype(np.float32), V.astype(np.float32)
    return F, V, 0.1


def quant_weights(kind, M, seed=0):
    """'dirichlet': random weights on the simplex; 'half': every second member has weight 0 (M >= 2)."""
    rs = np.random.RandomState(20000 + M + seed)
    w = rs.dirichlet(np.ones(M))
    if kind == "half" and M >= 2:
        w[1::2] = 0.0
        w /= w.sum()
    return w


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def mixture_residual(y, q, F, V, sigma, wm):
    """(|G(y) - q|, the bound on it) by the contract's G and density, per level and entry."""
    F = np.asarray(F).astype(np.float64)
    keep = np.arange(F.shape[0]) if wm is None else np.flatnonzero(wm > 0.0)
    s2 = sigma ** 2 + (0.0 if V is None else np.asarray(V).astype(np.float64)[keep]) + np.zeros_like(F[keep])
    G, g = pq.mixture_cdf(y, F[keep][:, None, :], np.sqrt(s2)[:, None, :], None if wm is None else wm[keep])
    return np.abs(G - np.asarray(q, dtype=np.float64)[:, None]), pq.residual_bound(y, g, F.shape[0])


# ------------------------------------------------------------------------------------------ the header and the ABI
def test_quantile_header_is_bound_and_exported():
    _lib.build()
    L = _lib.lib()
    hdr = open(_lib.QUANT_HEADER).read()
    code = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)                   # the comment names the calls it refers to
    assert set(re.findall(r"\b(qn_[a-z_0-9]+)\s*\(", code)) == set(_lib.QUANT_FUNCTIONS)
    assert list(_lib.QUANT_FUNCTIONS) == ["qn_pred_quantile_workspace_bytes", "qn_pred_quantile"]
    funcs, consts = _lib.parse_header(hdr)
    assert funcs == _lib.QUANT_FUNCTIONS and consts == {"QN_QUANT_MAX_M": 16384, "QN_QUANT_MAX_Q": 16, "QN_QUANT_MAX_ITER": 128}
    others = set(_lib.FUNCTIONS) | set(_lib.PSIS_FUNCTIONS) | set(_lib.STACK_FUNCTIONS) | set(_lib.RANK_FUNCTIONS) | set(_lib.EV_FUNCTIONS)
    assert not set(_lib.QUANT_FUNCTIONS) & others and "qn_quantile.hip" in _lib.SOURCES
    vp, i32, i64, sz, f64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_size_t, ctypes.c_double
    assert _lib.QUANT_FUNCTIONS["qn_pred_quantile_workspace_bytes"] == (sz, [i64, i64, i32, i32])
    assert _lib.QUANT_FUNCTIONS["qn_pred_quantile"] == (i32, [vp, vp, i32, vp, i64, i64, f64, vp, i32, vp, vp, vp, sz, vp])
    for name, (restype, argtypes) in _lib.QUANT_FUNCTIONS.items():
        fn = getattr(L, name)
        assert (fn.restype, list(fn.argtypes)) == (restype, argtypes), name
    assert (_lib.QUANT_MAX_M, _lib.QUANT_MAX_Q, _lib.QUANT_MAX_ITER) == (pq.QN_QUANT_MAX_M, pq.QN_QUANT_MAX_Q, pq.QN_QUANT_MAX_ITER)


def test_refusals_need_no_device():
    _lib.build()
    L = _lib.lib()
    EINVAL = _lib.CONSTANTS["QN_EINVAL"]
    for emp in (0, 1):
        assert L.qn_pred_quantile_workspace_bytes(100, 7, 3, emp) > 0
        assert L.qn_pred_quantile_workspace_bytes(_lib.QUANT_MAX_M, 1 << 20, _lib.QUANT_MAX_Q, emp) > 0
        for args, word in (((0, 7, 3), b"members"), ((_lib.QUANT_MAX_M + 1, 7, 3), b"members"), ((100, 0, 3), b"entries"),
                           ((100, 7, 0), b"levels"), ((100, 7, _lib.QUANT_MAX_Q + 1), b"levels")):
            assert L.qn_pred_quantile_workspace_bytes(*args, emp) == 0, args
            assert word in L.qn_last_error(), (args, L.qn_last_error())

    def call(M=100, K=7, dtype=_lib.QN_F64, sigma=0.1, q=(0.5,), V=None, nullq=False):
        qa = (ctypes.c_double * len(q))(*q)
        return L.qn_pred_quantile(None, V, dtype, None, M, K, sigma, None if nullq else qa, len(q), None, None, None, 0, None)

    # the call itself, refused before any device pointer is touched (they are NULL)
    for kw, word in ((dict(M=0), b"members"), (dict(M=_lib.QUANT_MAX_M + 1), b"members"), (dict(K=0), b"entries"),
                     (dict(q=()), b"levels"), (dict(q=(0.5,) * 17), b"levels"), (dict(dtype=77), b"dtype"),
                     (dict(sigma=-1.0), b"sigma"), (dict(sigma=float("nan")), b"sigma"), (dict(sigma=float("inf")), b"sigma"),
                     (dict(q=(0.5, 1.5)), b"level 1"), (dict(q=(-0.1,)), b"level 0"), (dict(q=(float("nan"),)), b"level 0"),
                     (dict(q=(0.5, 0.0)), b"mixture mode"), (dict(q=(1.0,)), b"mixture mode"),
                     (dict(q=(0.0,), sigma=0.0, V=1), b"mixture mode"),           # V given: mixture mode even at sigma = 0
                     (dict(q=(1.1,), sigma=0.0), b"empirical mode"), (dict(nullq=True), b"NULL"),
                     (dict(), b"NULL"), (dict(q=(0.0, 1.0), sigma=0.0), b"NULL")):  # legal shapes and levels: the NULL F is what is left
        assert call(**kw) == EINVAL, kw
        assert word in L.qn_last_error(), (kw, L.qn_last_error())


# ------------------------------------------------------------------------------------------ empirical mode
@pytest.mark.parametrize("M", MS)
def test_equal_weights_are_np_quantile_bit_for_bit(M):
    q = EMP_LEVELS[8] + [0.3333, 0.999]
    for kind in ("cont", "ties", "f32"):
        F, _, _ = quant_inputs(kind, M, 5)
        got = pq.empirical_quantiles(F, q)
        ref = np.quantile(F.astype(np.float64), q, axis=0)
        assert np.array_equal(bits(got), bits(ref)), (M, kind)
        if kind == "ties" and M >= 21:
            assert len(np.unique(F[:, 0])) < M                          # it does have ties
        assert np.array_equal(bits(pq.pred_quantiles_ref(F, q, 0.0)), bits(ref))


@pytest.mark.parametrize("M", MS)
def test_weighted_positions_reduce_to_the_equal_weight_ones(M):
    q = EMP_LEVELS[8]
    for kind in ("cont", "ties"):
        F, _, _ = quant_inputs(kind, M, 5)
        ref = pq.empirical_quantiles(F, q)
        got = pq.empirical_quantiles(F, q, np.full(M, 1.0 / M))
        # the positions (i - 1) / (n - 1) come out of a running sum of M terms: M eps on p, times the largest gap
        assert np.all(np.abs(got - ref) <= 1e-12 * np.abs(F).max()), (M, kind, np.abs(got - ref).max())
        assert np.array_equal(bits(got[[0, -1]]), bits(ref[[0, -1]]))   # the ends are the extreme members exactly


def test_weighted_quantile_by_hand_and_zero_weights_are_skipped():
    # three members 1, 2, 4 with weights .2, .5, .3: S = .2, .7, 1; p = (0, .35, .75) / .75
    F = np.array([[2.0], [4.0], [1.0]])
    w = np.array([0.5, 0.3, 0.2])
    p = np.array([0.0, 0.35, 0.75]) / 0.75
    got = pq.empirical_quantiles(F, [0.0, p[1] / 2, p[1], 0.5 * (p[1] + 1.0), 1.0], w)[:, 0]
    assert np.allclose(got, [1.0, 1.5, 2.0, 3.0, 4.0], rtol=1e-15)
    for M in (2, 21, 65):
        F, _, _ = quant_inputs("ties", M, 5)
        w = quant_weights("half", M)
        G = F.copy()
        G[w == 0.0] = np.nan                                            # what a member without weight holds plays no part
        a = pq.empirical_quantiles(G, EMP_LEVELS[8], w)
        assert np.all(np.isfinite(a))
        assert np.array_equal(bits(a), bits(pq.empirical_quantiles(F[w > 0.0], EMP_LEVELS[8], w[w > 0.0])))
    one = np.zeros(5)
    one[3] = 1.0
    F, _, _ = quant_inputs("cont", 5, 4)
    assert np.array_equal(pq.empirical_quantiles(F, [0.0, 0.4, 1.0], one), np.tile(F[3], (3, 1)))      # one surviving member


def test_ties_in_weighted_mode_follow_member_order():
    # two tied members: the earlier one comes first, so its weight decides where the plateau starts
    F = np.array([[1.0], [2.0], [2.0], [3.0]])
    a = pq.empirical_quantiles(F, [0.3], np.array([0.1, 0.6, 0.1, 0.2]))[0, 0]
    b = pq.empirical_quantiles(F, [0.3], np.array([0.1, 0.1, 0.6, 0.2]))[0, 0]
    assert a != b and 1.0 < a < 2.0 and 1.0 < b <= 2.0


# ------------------------------------------------------------------------------------------ mixture mode
def _bisect(q, f, s, w, n=200):
    """200 plain bisections on G(y) = q with scipy's erfc, from a bracket that holds the root."""
    lo = np.full(q.shape + f.shape[1:], (f - 40.0 * s).min())
    hi = np.full_like(lo, (f + 40.0 * s).max())
    for _ in range(n):
        mid = 0.5 * (lo + hi)
        G = ((0.5 * erfc(-(mid[None] - f[:, None]) / s[:, None] / np.sqrt(2.0))) * w[:, None, None]).sum(axis=0)
        up = G < q[:, None]
        lo, hi = np.where(up, mid, lo), np.where(up, hi, mid)
    return 0.5 * (lo + hi)


@pytest.mark.parametrize("M", MS)
def test_mixture_roots_against_plain_bisection(M):
    K = 3
    q = np.array(MIX_LEVELS[8] + [0.5001, 0.4999])
    worst = 0.0
    for kind, wkind, Vuse in (("cont", None, True), ("bimodal", "dirichlet", True), ("f32", "half", False), ("bimodal", None, False)):
        F, V, sigma = quant_inputs(kind, M, K)
        V = V if Vuse else None
        wm = None if wkind is None else quant_weights(wkind, M)
        y, iters = pq.mixture_quantiles(F, q, sigma, V, wm, return_iters=True)
        res, bound = mixture_residual(y, q, F, V, sigma, wm)
        worst = max(worst, float((res / bound).max()))
        assert np.all(res <= bound), (M, kind, float((res / bound).max()))
        assert iters.min() >= 1 and iters.max() <= pq.QN_QUANT_MAX_ITER
        keep = np.arange(M) if wm is None else np.flatnonzero(wm > 0.0)
        f = F.astype(np.float64)[keep]
        s = np.sqrt(sigma ** 2 + (V.astype(np.float64)[keep] if V is not None else np.zeros_like(f)))
        yb = _bisect(q, f, s, np.full(M, 1.0 / M) if wm is None else wm[keep])
        resb, boundb = mixture_residual(yb, q, F, V, sigma, wm)
        _, g = pq.mixture_cdf(y, f[:, None, :], s[:, None, :], None if wm is None else wm[keep])
        # two points whose G lies within its bound of q are no further apart than the two bounds over the density
        assert np.all(np.abs(y - yb) * g <= 2.0 * (bound + np.maximum(resb, boundb))), (M, kind)
    print(f"M={M}: worst residual / bound {worst:.2f}")


def test_mixture_closed_forms():
    z = pq.inv_normal_cdf(MIX_LEVELS[8])
    # one member, and identical members: the Gaussian quantile f + s z
    for M in (1, 7):
        F = np.tile(np.array([[1.5, -2.0, 0.0]]), (M, 1))
        V = np.tile(np.array([[0.3, 0.0, 1.0]]), (M, 1))
        y = pq.mixture_quantiles(F, MIX_LEVELS[8], 0.5, V)
        ref = F[0][None, :] + np.sqrt(0.25 + V[0])[None, :] * z[:, None]
        assert np.allclose(y, ref, rtol=1e-13, atol=1e-14)
    # two far modes of equal weight: the level 0.25 is the median of the lower one
    F = np.array([[0.0], [100.0]])
    y = pq.mixture_quantiles(F, [0.25, 0.75], 1.0)
    assert np.allclose(y[:, 0], [0.0, 100.0], atol=1e-13)
    # a level in the gap stops within the cap and meets the bound
    y, it = pq.mixture_quantiles(F, [0.5, 0.5 + 1e-9], 1.0, return_iters=True)
    res, bound = mixture_residual(y, [0.5, 0.5 + 1e-9], F, None, 1.0, None)
    assert np.all(res <= bound) and it[0] <= pq.QN_QUANT_MAX_ITER and abs(y[0, 0] - 50.0) < 1.0


def test_nan_rules_and_bad_weights():
    F, V, sigma = quant_inputs("cont", 21, 6)
    q = MIX_LEVELS[3]
    ref, it = pq.pred_quantiles_ref(F, q, sigma, V, return_iters=True)
    G, W = F.copy(), V.copy()
    G[4, 1] = np.nan
    W[7, 3] = -sigma ** 2                                               # s^2 = 0
    W[2, 5] = np.inf
    got, it2 = pq.pred_quantiles_ref(G, q, sigma, W, return_iters=True)
    assert np.all(np.isnan(got[:, [1, 3, 5]])) and np.array_equal(bits(got[:, [0, 2, 4]]), bits(ref[:, [0, 2, 4]]))
    assert np.all(it2[[1, 3, 5]] == 0) and np.array_equal(it2[[0, 2, 4]], it[[0, 2, 4]])
    emp = pq.pred_quantiles_ref(G, EMP_LEVELS[3], 0.0)
    assert np.all(np.isnan(emp[:, 1])) and np.array_equal(bits(emp[:, 0]), bits(np.quantile(F[:, 0], EMP_LEVELS[3])))
    for bad in (-1e-3, np.nan, np.inf):
        w = np.full(21, 1.0 / 21)
        w[5] = bad
        assert np.all(np.isnan(pq.pred_quantiles_ref(F, q, sigma, V, w))) and np.all(np.isnan(pq.pred_quantiles_ref(F, q, 0.0, None, w)))
    assert np.all(np.isnan(pq.pred_quantiles_ref(F, q, sigma, V, np.zeros(21))))
    for kw in (dict(q=[0.0]), dict(q=[1.0]), dict(q=[np.nan]), dict(q=[]), dict(q=[0.5] * 17), dict(sigma=-1.0)):
        with pytest.raises(ValueError):
            pq.pred_quantiles_ref(F, kw.get("q", q), kw.get("sigma", sigma), V)
    with pytest.raises(ValueError):
        pq.pred_quantiles_ref(F, [1.5], 0.0)


# ------------------------------------------------------------------------------------------ interval summary
def test_interval_summary_by_hand():
    lo = np.array([[0.0], [0.0], [1.0], [1.0]])
    hi = np.array([[1.0], [2.0], [2.0], [3.0]])
    y = np.array([[0.5], [3.0], [1.0], [0.0]])
    s = scoring.interval_summary(lo, hi, y, 0.9)
    assert s["n"] == 4 and s["width"] == 1.5 and s["coverage"] == 0.5
    assert abs(s["interval_score"] - (1.5 + 20.0 * (0.0 + 1.0 + 0.0 + 1.0) / 4)) < 1e-14
    with pytest.raises(ValueError):
        scoring.interval_summary(lo, hi, y[:3], 0.9)
    with pytest.raises(ValueError):
        scoring.interval_summary(lo, hi, y, 1.0)
