"""CPU: the numpy contract of stacking (`quinn_amd/stacking.py`, the authority of `qn_group_lpd`, `qn_stack_weights` and
`qn_pred_score_w`) against known optima and its own structure; the header include/quinn_amd_stack.h against the binding and
the library; the refusals that need no device.  Every randomised input of tests/test_gpu_stacking.py is generated HERE
(`stack_L`, `disjoint_L`, `special_L`, `lpd_data`, `weights_data`) and checked to stop by its gap well inside the iteration
cap and to drop nothing, so that the GPU tests cannot pass by hitting the cap."""
import ctypes
import os
import re

import numpy as np
import pytest

from quinn_amd import _lib, stacking
from test_pred_score_cpu import score_np

LD = np.longdouble
TOL, MAX_ITER = stacking.DEFAULT_TOL, stacking.DEFAULT_MAX_ITER
STACK_SHAPES = ((1, 7), (2, 1), (5, 257), (65, 1000), (1024, 33))       # (G, K) of the GPU parity test
DISJOINT_SIZES = (3, 70, 1, 259, 64)


def stack_L(G, K, seed=0):
    """L `[G, K]`: the targets z_k come from three well separated unit clusters at -6, 0 and 6 (shares 0.5, 0.3, 0.2); the
    first min(G, 3) groups predict one cluster each, N(c_g, 1) -- every other group is a degraded copy of one of them, its log
    density lower by d_g in [0.5, 3] and by half-normal noise per entry: groups of deliberately different quality.  A degraded
    group is dominated on every entry, so its weight decays geometrically, the supports of the good ones barely overlap, and
    EM gets to a gap of 1e-3 in tens of iterations rather than the thousands it needs on groups of nearly equal quality."""
    rs = np.random.RandomState(100 * G + K + seed)
    c = np.array([-6.0, 0.0, 6.0])[:min(G, 3)]
    z = np.array([-6.0, 0.0, 6.0])[rs.choice(3, size=K, p=[0.5, 0.3, 0.2])] + rs.randn(K)
    good = -0.5 * (z[None] - c[:, None]) ** 2 - 0.5 * np.log(2 * np.pi)
    L = good[np.arange(G) % len(c)] - rs.uniform(0.5, 3.0, size=(G, 1)) - np.abs(rs.randn(G, K))
    L[:len(c)] = good
    return L


def slow_L(G=5, K=257):
    """Groups of nearly equal quality -- targets z_k ~ N(0, 1), group g predicts N(b_g, s_g^2) with a random bias and scale -- on
    which EM needs hundreds of iterations (567 at the defaults): the case that spans several blocks of launches."""
    rs = np.random.RandomState(100 * G + K)
    z = rs.randn(K)
    b = 1.5 * rs.randn(G)
    s = np.exp(0.4 * rs.randn(G))
    b[::7], s[::7] = 0.1 * b[::7], 1.0 + 0.1 * (s[::7] - 1.0)
    return -0.5 * ((z[None] - b[:, None]) / s[:, None]) ** 2 - np.log(s)[:, None] - 0.5 * np.log(2 * np.pi)


def disjoint_L(sizes=DISJOINT_SIZES):
    """Group g has L = 0 on its own block of sizes[g] entries and -Inf elsewhere: the optimum is w_g = sizes[g] / K."""
    K = int(np.sum(sizes))
    L = np.full((len(sizes), K), -np.inf)
    lo = 0
    for g, n in enumerate(sizes):
        L[g, lo:lo + n] = 0.0
        lo += n
    return L


def special_L():
    """`stack_L(5, 257)` with a NaN, a +Inf, two columns that are -Inf throughout and one that is non-finite throughout:
    n_nonfinite = 2 + 5 = 7, n_dropped = 3."""
    L = stack_L(5, 257, seed=3)
    L[1, 4] = np.nan
    L[3, 200] = np.inf
    L[:, 64], L[:, 256] = -np.inf, -np.inf
    L[:, 100] = [np.nan, np.inf, np.nan, np.nan, np.inf]
    return L


def lpd_data(M, K, dtype, with_v, seed=0):
    """(F, V or None, y) as tests/test_psis_cpu.py's `loo_data`: members spread by half a predictive standard deviation."""
    rs = np.random.RandomState(1000 * M + K + seed)
    mu = rs.randn(K) * 2.0
    V = rs.uniform(0.1, 0.5, size=(M, K)).astype(dtype) if with_v else None
    F = (mu + 0.4 * rs.randn(M, K) + 0.3 * rs.randn(M, 1)).astype(dtype)
    return F, V, mu + 0.8 * rs.randn(K)


def weights_data(M, seed=0):
    """Random member weights on the simplex, a fifth of them exactly 0 (M >= 5)."""
    rs = np.random.RandomState(7 * M + seed)
    w = rs.gamma(0.7, size=M)
    if M >= 5:
        w[rs.permutation(M)[:M // 5]] = 0.0
    return w / w.sum()


# ------------------------------------------------------------------------------------------ the inputs of the GPU tests
@pytest.mark.parametrize("G,K", STACK_SHAPES)
def test_gpu_inputs_stop_by_gap(G, K):
    r = stacking.stack_weights(stack_L(G, K), TOL, MAX_ITER)
    print(f"G={G} K={K}: iters {r['iters']} gap {r['gap']:.2e} obj {r['obj']:.6f} (equal {r['obj_equal']:.6f})")
    assert r["gap"] <= TOL and r["iters"] <= MAX_ITER // 4
    assert r["n_dropped"] == 0 and r["n_nonfinite"] == 0 and r["n_kept"] == K


def test_gpu_special_inputs_stop_by_gap():
    for L, dropped, nonfinite in ((disjoint_L(), 0, 0), (special_L(), 3, 7), (slow_L(), 0, 0)):
        r = stacking.stack_weights(L, TOL, MAX_ITER)
        print(f"{L.shape}: iters {r['iters']} gap {r['gap']:.2e}")
        assert r["gap"] <= TOL and r["iters"] <= MAX_ITER // 4
        assert (r["n_dropped"], r["n_nonfinite"], r["n_kept"]) == (dropped, nonfinite, L.shape[1] - dropped)


# ------------------------------------------------------------------------------------------ properties of the contract
def test_objective_is_monotone_and_gap_certifies():
    for G, K in ((5, 257), (65, 1000)):
        r = stacking.stack_weights(stack_L(G, K), TOL, MAX_ITER, trace=True)
        assert np.all(np.diff(r["objs"]) >= -1e-12 * np.abs(r["objs"][:-1]))
        assert r["gaps"][-1] <= TOL and np.all(r["gaps"][:-1] > TOL)
        assert r["obj"] == r["objs"][-1] and r["obj_equal"] == r["objs"][0] and r["iters"] == len(r["objs"]) - 1
        assert np.all(r["objs"][-1] - r["objs"] <= r["gaps"] + 1e-9)         # the gap bounds obj(w*) - obj(w) >= obj(end) - obj(w)
        assert abs(r["w"].sum() - 1) < 1e-14 and np.all(r["w"] >= 0)


def test_disjoint_support_is_solved_in_one_iteration():
    r = stacking.stack_weights(disjoint_L(), TOL, MAX_ITER)
    assert r["iters"] == 1
    assert np.max(np.abs(r["w"] - np.array(DISJOINT_SIZES) / np.sum(DISJOINT_SIZES))) <= 1e-15


def test_dominating_group_takes_the_weight():
    L = stack_L(5, 257)
    L[2] = L.max(axis=0) + 0.5
    r = stacking.stack_weights(L, 1e-9, MAX_ITER)
    assert r["gap"] <= 1e-9 and r["w"][2] > 1 - 1e-9


def test_identical_groups_share_one_weight():
    L = stack_L(5, 257)
    r5 = stacking.stack_weights(L, 1e-8, 50000)
    r6 = stacking.stack_weights(np.concatenate([L, L[1:2]]), 1e-8, 50000)
    assert r5["gap"] <= 1e-8 and r6["gap"] <= 1e-8
    merged = np.append(np.delete(r6["w"], 5), 0.0)[:5]
    merged[1] += r6["w"][5]
    print("identical groups: |dw|", np.max(np.abs(merged - r5["w"])), "dobj", r6["obj"] - r5["obj"])
    assert abs(r6["obj"] - r5["obj"]) <= 2e-8                   # both certified to 1e-8 of the same optimum
    assert np.max(np.abs(merged - r5["w"])) < 1e-3


def test_nonfinite_and_dropped_entries():
    L = special_L()
    r = stacking.stack_weights(L, TOL, MAX_ITER)
    keep = np.ones(257, dtype=bool)
    keep[[64, 100, 256]] = False
    clean = np.where(np.isnan(L) | np.isposinf(L), -np.inf, L)[:, keep]            # NaN / +Inf: density 0
    c = stacking.stack_weights(clean, TOL, MAX_ITER)
    assert c["n_nonfinite"] == 0 and c["n_dropped"] == 0
    assert np.array_equal(r["w"], c["w"]) and r["obj"] == c["obj"] and r["iters"] == c["iters"]
    e = stacking.stack_weights(np.full((3, 4), -np.inf))
    assert e["n_kept"] == 0 and np.all(e["w"] == 1 / 3) and e["obj"] == 0 and e["iters"] == 0
    one = stacking.stack_weights(stack_L(1, 7))
    assert one["iters"] == 0 and one["w"][0] == 1.0


def test_group_lpd_is_the_equal_weight_lppd_of_the_slice():
    F, V, y = lpd_data(7, 65, np.float64, True)
    L = stacking.group_lpd(F, y, 0.3, [0, 1, 3, 7], V)
    for g, (lo, hi) in enumerate(((0, 1), (1, 3), (3, 7))):
        if hi - lo >= 2:
            assert np.max(np.abs(L[g] - score_np(F[lo:hi], V[lo:hi], y, 0.3, crps=False)[0])) < 1e-13
    s2 = 0.3 ** 2 + V[0]
    assert np.max(np.abs(L[0] - (-0.5 * (y - F[0]) ** 2 / s2 - 0.5 * np.log(2 * np.pi * s2)))) < 1e-13
    F[4, 9] = np.nan
    Lb = stacking.group_lpd(F, y, 0.3, [0, 1, 3, 7], V)
    assert np.isnan(Lb[2, 9]) and np.isnan(Lb).sum() == 1 and np.array_equal(np.isnan(Lb) | (Lb == L), np.ones_like(L, dtype=bool))


@pytest.mark.parametrize("M,K", [(2, 1), (33, 129), (130, 9)])
def test_weighted_rows_at_equal_weights_are_pred_score(M, K):
    """Against the independent equal-weight restatement of tests/test_pred_score_cpu.py."""
    for with_v, sigma in ((False, 0.3), (True, 0.05)):
        F, V, y = lpd_data(M, K, np.float64, with_v)
        got = stacking.weighted_rows(F, y, sigma, np.full(M, 1.0 / M), V)
        ref = score_np(F, V, y, sigma)
        for r in range(6):
            assert np.max(np.abs(got[r] - ref[r])) <= 1e-12 * np.max(np.abs(ref[r])), (r, with_v)


def test_weighted_rows_rules():
    F, V, y = lpd_data(9, 40, np.float64, True)
    w = weights_data(9)
    assert (w == 0).sum() == 1
    rows = stacking.weighted_rows(F, y, 0.2, w, V)
    Fn = F.copy()
    Fn[w == 0] = np.nan                                         # a zero-weight member is never looked at
    assert np.array_equal(stacking.weighted_rows(Fn, y, 0.2, w, V), rows)
    assert np.array_equal(stacking.weighted_rows(F[w > 0], y, 0.2, w[w > 0], V[w > 0]), rows)
    hot = np.zeros(9)
    hot[4] = 1.0
    one = stacking.weighted_rows(F, y, 0.2, hot, V)
    s2 = 0.2 ** 2 + V[4]
    assert np.all(one[1] == 0) and np.all(one[5] == 0) and np.array_equal(one[4], F[4])
    assert np.max(np.abs(one[3] - (stacking._crps_a(y - F[4], s2, np.float64) - 0.5 * stacking._crps_a(0 * y, 2 * s2, np.float64)))) < 1e-15
    w[2] = -w[2] if w[2] else -0.1
    assert np.isnan(stacking.weighted_rows(F, y, 0.2, w, V)).all()
    mom = stacking.weighted_rows(F, None, 0.0, weights_data(9))
    assert np.isnan(mom[:4]).all() and np.max(np.abs(mom[4] - weights_data(9) @ F)) < 1e-14
    assert np.array_equal(stacking.member_weights([0.5, 0.2, 0.3], [0, 1, 3, 7]), [0.5, 0.1, 0.1, 0.075, 0.075, 0.075, 0.075])


# ------------------------------------------------------------------------------------------ the ABI without a device
def test_stack_header_is_bound_and_exported():
    """include/quinn_amd_stack.h declares the six entry points; the binding follows from it and the library exports them."""
    _lib.build()
    L = _lib.lib()
    hdr = open(_lib.STACK_HEADER).read()
    assert set(re.findall(r"\b(qn_[a-z_0-9]+)\s*\(", hdr)) == set(_lib.STACK_FUNCTIONS) | {"qn_last_error"}
    assert list(_lib.STACK_FUNCTIONS) == ["qn_group_lpd_workspace_bytes", "qn_group_lpd", "qn_stack_weights_workspace_bytes",
                                          "qn_stack_weights", "qn_pred_score_w_workspace_bytes", "qn_pred_score_w"]
    assert not set(_lib.STACK_FUNCTIONS) & (set(_lib.FUNCTIONS) | set(_lib.PSIS_FUNCTIONS))
    assert os.path.exists(os.path.join(_lib.CSRC, "qn_stack.hip")) and "qn_stack.hip" in _lib.SOURCES
    vp, i32, i64, f64, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double, ctypes.c_size_t
    assert _lib.STACK_FUNCTIONS["qn_group_lpd"] == (i32, [vp, vp, i32, vp, i64, i64, f64, vp, i64, vp, vp, sz, vp])
    assert _lib.STACK_FUNCTIONS["qn_group_lpd_workspace_bytes"] == (sz, [i64, i64, i64])
    assert _lib.STACK_FUNCTIONS["qn_stack_weights"] == (i32, [vp, i64, i64, f64, i64, i64, i64, vp, vp, vp, sz, vp])
    assert _lib.STACK_FUNCTIONS["qn_stack_weights_workspace_bytes"] == (sz, [i64, i64])
    assert _lib.STACK_FUNCTIONS["qn_pred_score_w"] == (i32, [vp, vp, i32, vp, vp, i64, i64, f64, i32, vp, vp, sz, vp])
    assert _lib.STACK_FUNCTIONS["qn_pred_score_w_workspace_bytes"] == (sz, [i64, i64, i32])
    for name, (restype, argtypes) in _lib.STACK_FUNCTIONS.items():
        fn = getattr(L, name)
        assert (fn.restype, list(fn.argtypes)) == (restype, argtypes), name
    assert _lib.STACK_MAX_G == 1024 and _lib.STACK_NSTATUS == len(stacking.STATUS)


def test_abi_needs_no_device():
    _lib.build()
    L = _lib.lib()
    EINVAL, EWORKSPACE = -1, -2
    assert L.qn_stack_weights_workspace_bytes(5, 257) > 0 and L.qn_stack_weights_workspace_bytes(1024, 1) > 0
    for args in ((0, 7), (1025, 7), (5, 0), (5, 2 ** 31 + 1)):
        assert L.qn_stack_weights_workspace_bytes(*args) == 0 and L.qn_last_error(), args
    assert L.qn_group_lpd_workspace_bytes(7, 65, 3) > 0 and L.qn_group_lpd_workspace_bytes(1, 1, 1) > 0
    for args in ((0, 65, 1), (7, 0, 3), (7, 65, 0), (7, 65, 8)):
        assert L.qn_group_lpd_workspace_bytes(*args) == 0 and L.qn_last_error(), args
    assert L.qn_pred_score_w_workspace_bytes(1, 1, 31) > 0
    for args in ((0, 5, 31), (5, 0, 31), (5, 5, 0), (5, 5, 32)):
        assert L.qn_pred_score_w_workspace_bytes(*args) == 0 and L.qn_last_error(), args
    buf = (ctypes.c_double * 8)()
    p = ctypes.addressof(buf)                        # never dereferenced: every call below is refused first
    off = (ctypes.c_int64 * 4)(0, 1, 3, 6)           # does not end at M = 7

    def stack(L_=p, G=5, K=257, tol=1e-3, max_iter=10, t0=0, n=4, w=p, status=p, ws=p, nbytes=1 << 30):
        return L.qn_stack_weights(L_, G, K, tol, max_iter, t0, n, w, status, ws, nbytes, None)

    for kw in ({"G": 0}, {"G": 1025}, {"K": 0}, {"tol": -1.0}, {"tol": float("nan")}, {"max_iter": -1}, {"t0": -1}, {"n": 0},
               {"L_": None}, {"w": None}, {"status": None}, {"ws": None}):
        assert stack(**kw) == EINVAL and L.qn_last_error(), kw
    assert stack(nbytes=8) == EWORKSPACE and b"workspace" in L.qn_last_error()

    def lpd(F=p, V=None, dtype=0, Y=p, M=7, K=65, sigma=0.1, offsets=ctypes.addressof(off), G=3, out=p, ws=p, nbytes=1 << 20):
        return L.qn_group_lpd(F, V, dtype, Y, M, K, sigma, offsets, G, out, ws, nbytes, None)

    for kw in ({"M": 0}, {"K": 0}, {"G": 0}, {"G": 8}, {"dtype": 2}, {"sigma": -0.1}, {"sigma": float("inf")}, {"sigma": 0.0},
               {"F": None}, {"Y": None}, {"offsets": None}, {"out": None}, {"ws": None}, {}):
        assert lpd(**kw) == EINVAL and L.qn_last_error(), kw              # {}: the offsets end at 6, not 7
    assert b"offsets" in L.qn_last_error()
    assert lpd(nbytes=8) == EWORKSPACE

    def scorew(F=p, V=None, dtype=0, Y=p, wm=p, M=5, K=5, sigma=0.1, what=31, out=p, ws=p, nbytes=1 << 20):
        return L.qn_pred_score_w(F, V, dtype, Y, wm, M, K, sigma, what, out, ws, nbytes, None)

    for kw in ({"M": 0}, {"K": 0}, {"what": 0}, {"what": 32}, {"dtype": 2}, {"sigma": -0.1}, {"sigma": 0.0}, {"F": None}, {"Y": None},
               {"wm": None}, {"out": None}, {"ws": None}):
        assert scorew(**kw) == EINVAL and L.qn_last_error(), kw
    assert scorew(nbytes=8) == EWORKSPACE
