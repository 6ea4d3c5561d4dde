"""The sample-space proposal kernels of the device AMCMC engine (csrc/qn_mcmc.hip) against exact numpy references.

`qn_mcmc_propose_hist_block` leaves the float16 coefficients it multiplied with in the caller's `coef` buffer, the single-step
kernel forms the same coefficients for the same absolute step, and `qn_mcmc_propose(cur = NULL)` writes the elementwise normals of
any step: so both history products can be recomputed on the host from device-visible inputs, and the tolerances follow from the
arithmetic (float32 accumulation of exact float16 x float16 products on the matrix cores; float64 fma in the single-step kernel).
Nothing here is statistical except the moment check of the coefficients (fixed seed).

Everything a kernel must not use is NaN (history rows >= K, pad columns [p, pstride), wsnap[K:]) and every output is pre-filled
with NaN: the engine hands over uninitialised memory there.

Only the GPU tests carry the `gpu` mark (not the module): the self-check of the reference at the end runs without a device."""
import numpy as np
import pytest

gpu = pytest.mark.gpu

TB = 64                     # qn_mcmc_hist_block_steps(), asserted on the device
SEED = 1234
CHAIN0 = 5
S_LR = 0.0371
S_ISO = 0.29
SCALES = (1.0, 64.0, 2.0 ** -3)
ORDER = (2, 0, 1)


def _ceil4(p):
    return (p + 3) // 4 * 4


def _kstride(kcap):
    return (kcap + 7) // 8 * 8


# (K per chain, kcap, ksnap or None): kcap from {K_max, K_max + 3, 61}: kstride != kcap and K == kcap both occur
K_CASES = [
    ((0, 1, 7), 61, None), ((0, 1, 7), 7, None),
    ((8, 9, 15), 18, None), ((8, 9, 15), 15, None),
    ((16, 17, 40), 40, None), ((16, 17, 40), 61, None),
    ((127, 128, 129), 129, None), ((127, 128, 129), 132, None),
    ((136, 257, 300), 300, None), ((136, 257, 300), 303, None),
    ((2047, 2048, 4100), 4100, None), ((2047, 2048, 4100), 4103, None),
    ((9, 61, 20), 61, (9, 66, 20)),                                        # ksnap = kcap + 5: clamped to kcap
]
P_LIST = [1, 2, 3, 4, 5, 7, 127, 128, 129, 130, 511, 512, 513, 515, 1030]


def _cases():
    """(id, Ks, kcap, ksnap, p, pstride, use_hscale): big K only with small p, big p only with K <= 300."""
    out = []
    for Ks, kcap, ksnap in K_CASES:
        for p in (5, 130):
            out.append((f"K{'_'.join(map(str, Ks))}-kcap{kcap}-p{p}", Ks, kcap, ksnap, p, _ceil4(p), True))
    for i, p in enumerate(P_LIST):
        pstride = _ceil4(p) + (8 if p in (5, 513) else 0)
        out.append((f"p{p}-ps{pstride}", (40, 129, 300), 300 if i % 2 else 303, None, p, pstride, True))
    out.append(("nohscale-p130", (40, 129, 300), 303, None, 130, 132, False))
    return out


CASES = _cases()
CASE_IDS = [c[0] for c in CASES]


def _make(seed, Ks, kcap, ksnap, p, pstride, use_hscale=True):
    """Host inputs of one case; NaN wherever the kernels must not look."""
    rs = np.random.RandomState(seed)
    C = len(Ks)
    S = np.array(SCALES[:C] if use_hscale else (1.0,) * C)
    hist = (rs.uniform(512.0, 2048.0, (C, kcap, pstride)) * rs.choice([-1.0, 1.0], (C, kcap, pstride))).astype(np.float16)
    wsnap = rs.uniform(1.0, 4.0, (C, kcap)).astype(np.float32)
    mean = rs.randn(C, p) * 1024.0 / S[:, None]                             # the size of the rows divided by S
    cur = 50.0 * rs.randn(C, p)
    hist[:, :, p:] = np.nan
    for c, K in enumerate(Ks):
        hist[c, K:] = np.nan
        wsnap[c, K:] = np.nan
    return dict(Ks=tuple(Ks), kcap=kcap, p=p, pstride=pstride, S=S, use_hscale=use_hscale, hist=hist, wsnap=wsnap, mean=mean, cur=cur,
                ksnap=np.array(ksnap if ksnap is not None else Ks, dtype=np.int32))


def block_reference(coef, hist, mean, S, Ks, p, s_lr, drop_row=None, swap_cols=None, stop_short=False, drop_chunk=None):
    """delta_ref and the magnitude sum of its terms, per chain in float64:
        delta_ref[c,t,j] = s_lr (sum_{k<K} coef[c,t,k] hist[c,k,j] / S_c - (sum_{k<K} coef[c,t,k]) mean[c,j])
        mag[c,t,j]       = sum_k |coef hist| / S + |mean_j| sum_k |coef|
    The keyword arguments recompute it WRONG on purpose (self-check at the end of the file): one history row left out, two
    adjacent columns swapped, the sum stopped at K - 1, one 128-row chunk left out."""
    C, tb = coef.shape[0], coef.shape[1]
    ref = np.zeros((C, tb, p))
    mag = np.zeros((C, tb, p))
    for c, K in enumerate(Ks):
        keep = np.ones(K, dtype=bool)
        if drop_row is not None and K > 0:
            keep[drop_row % K] = False
        if stop_short and K > 0:
            keep[K - 1] = False
        if drop_chunk is not None and K > 128 * drop_chunk:
            keep[128 * drop_chunk:128 * (drop_chunk + 1)] = False
        cf = coef[c, :, :K].astype(np.float64)[:, keep]
        h = hist[c, :K, :p].astype(np.float64)[keep]
        if swap_cols is not None and swap_cols + 1 < p:
            h = h.copy()
            h[:, [swap_cols, swap_cols + 1]] = h[:, [swap_cols + 1, swap_cols]]
        ref[c] = s_lr * (cf @ h / S[c] - cf.sum(axis=1)[:, None] * mean[c][None, :])
        mag[c] = np.abs(cf) @ np.abs(h) / S[c] + np.abs(cf).sum(axis=1)[:, None] * np.abs(mean[c])[None, :]
    return ref, mag


def block_bound(ref, mag, Ks, s_lr):
    """Forward bound of a float32 accumulation of K exact float16 x float16 products in any order, 2^-23 per operation (covers a
    non-nearest internal rounding of the matrix unit), + 16 for the padded step; a few 2^-53 |ref| for the final float64
    operations.  (The float64 reference's own error, K 2^-53 mag, is 2^-30 of this.)"""
    K = np.array(Ks, dtype=np.float64)[:, None, None]
    return s_lr * (K + 16.0) * 2.0 ** -23 * mag + 4 * 2.0 ** -53 * np.abs(ref)


def _worst(err, bound):
    """largest err / bound and where; an element with bound 0 (K = 0) must have err 0"""
    assert not np.isnan(err).any(), "NaN in the result: an element was not written, or pad / stale memory was used"
    assert (err[bound == 0] == 0).all()
    r = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), 0.0)
    i = np.unravel_index(np.argmax(r), r.shape)
    return float(r[i]), tuple(int(v) for v in i)


# ------------------------------------------------------------------------------------------------------------ device helpers
def _L():
    from quinn_amd import _lib
    L = _lib.lib()
    assert L.qn_mcmc_hist_block_steps() == TB
    return _lib, L


def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _nan_like(shape):
    import torch
    return torch.full(shape, float("nan"), dtype=torch.float64, device="cuda")


def _ptr(t):
    return None if t is None else t.data_ptr()


def _upload(d):
    g = {k: _dev(d[k]) for k in ("hist", "wsnap", "mean", "cur", "ksnap")}
    g["hscale"] = _dev(d["S"]) if d["use_hscale"] else None
    return g


def _run_block(d, g, step0=10, chain0=CHAIN0, order=None, step_ptr=None):
    """-> coef float16 [C, TB, kstride], delta float64 [C, TB, p] (numpy)"""
    import torch
    _lib, L = _L()
    C, kcap, p = len(d["Ks"]), d["kcap"], d["p"]
    ks = _kstride(kcap)
    nbytes = L.qn_mcmc_hist_block_coef_bytes(C, kcap)
    assert nbytes == C * TB * ks * 2
    coef = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device="cuda")              # float16 NaN everywhere
    delta = _nan_like((C, TB, p))
    od = _dev(np.array(order, dtype=np.int32)) if order is not None else None
    sp = _dev(np.array([step_ptr, -1], dtype=np.int64)) if step_ptr is not None else None
    _lib.check(L.qn_mcmc_propose_hist_block(g["hist"].data_ptr(), g["wsnap"].data_ptr(), g["ksnap"].data_ptr(), g["mean"].data_ptr(),
                                            _ptr(g["hscale"]), S_LR, S_ISO, C, chain0, p, d["pstride"], kcap, SEED,
                                            0 if step_ptr is not None else step0, _ptr(sp), coef.data_ptr(), delta.data_ptr(),
                                            _ptr(od), None), "propose_hist_block")
    torch.cuda.synchronize()
    return coef.cpu().numpy().view(np.float16).reshape(C, TB, ks), delta.cpu().numpy()


def _normals(C, p, step, chain0=CHAIN0):
    import torch
    _lib, L = _L()
    z = _nan_like((C, p))
    sp = _dev(np.array([step, -1], dtype=np.int64))
    _lib.check(L.qn_mcmc_propose(None, None, 0.0, C, chain0, p, SEED, sp.data_ptr(), z.data_ptr(), None), "propose")
    torch.cuda.synchronize()
    return z.cpu().numpy()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


# ------------------------------------------------------------------------------ 1. k_hist_block16 against the reference
@gpu
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_block_product_matches_float64_reference(case):
    name, Ks, kcap, ksnap, p, pstride, use_hscale = case
    d = _make(CASES.index(case), Ks, kcap, ksnap, p, pstride, use_hscale)
    coef, delta = _run_block(d, _upload(d), order=ORDER)
    for c, K in enumerate(Ks):                                                        # (k_hist_coef: zero beyond K up to kstride)
        assert np.isfinite(coef[c, :, :K].astype(np.float64)).all()
        assert (_bits(coef[c, :, K:]) == 0).all()
        if K == 0:
            assert (delta[c] == 0.0).all()                                            # exactly
    ref, mag = block_reference(coef, d["hist"], d["mean"], d["S"], Ks, p, S_LR)
    bound = block_bound(ref, mag, Ks, S_LR)
    r, at = _worst(np.abs(delta - ref), bound)
    print(f"\nhist_block16 {name}: max err/bound = {r:.4g} at (chain, t, col) = {at}")
    assert r <= 1.0, (name, r, at)


@gpu
def test_block_product_exact_contracts():
    """Bit for bit: the same call twice; with and without `order`; (step0 = 10, t = 7) against (step0 = 17, t = 0); step0 through
    step_ptr against step0 by value; chain b under chain0 = 5 against chain 5 + b under chain0 = 0."""
    Ks, kcap, p, pstride = (136, 257, 300), 303, 130, 132
    d = _make(77, Ks, kcap, None, p, pstride)
    g = _upload(d)
    c0, d0 = _run_block(d, g, step0=10, order=ORDER)
    for what, kw in (("twice", dict(step0=10, order=ORDER)), ("no order", dict(step0=10)), ("step_ptr", dict(step_ptr=10, order=ORDER))):
        c1, d1 = _run_block(d, g, **kw)
        assert np.array_equal(_bits(c0), _bits(c1)), what
        assert np.array_equal(_bits(d0), _bits(d1)), what
    c2, d2 = _run_block(d, g, step0=17, order=ORDER)
    assert np.array_equal(_bits(c0[:, 7]), _bits(c2[:, 0])) and np.array_equal(_bits(d0[:, 7]), _bits(d2[:, 0]))
    assert not np.array_equal(_bits(c0[:, 0]), _bits(c2[:, 0]))
    # eight chains under chain0 = 0 whose chains 5..7 are the three above (0..4: the same data again, other global ids)
    pick = [0, 1, 2, 0, 1, 0, 1, 2]
    d8 = dict(d, Ks=tuple(Ks[i] for i in pick), S=d["S"][pick])
    for k in ("hist", "wsnap", "mean", "cur", "ksnap"):
        d8[k] = d[k][pick]
    c8, dl8 = _run_block(d8, _upload(d8), step0=10, chain0=0, order=(7, 3, 0, 5, 1, 6, 2, 4))
    assert np.array_equal(_bits(c8[5:]), _bits(c0)) and np.array_equal(_bits(dl8[5:]), _bits(d0))
    assert not np.array_equal(_bits(c8[0]), _bits(c0[0]))                             # same data, another global chain id


# --------------------------------------------------------------------------------------------------------- 2. k_hist_coef
@gpu
def test_coefficients_follow_wsnap_exactly():
    """wsnap[k] = 2^(k % 5) against wsnap = 1: coef_a == 2^(k % 5) coef_b exactly (a power of two times a float32 rounds to float16
    as the float32 does, as long as neither side is subnormal or overflows): the wsnap indexing, per chain and row."""
    Ks, kcap, p = (40, 129, 300), 303, 5
    d = _make(5, Ks, kcap, None, p, 8)
    pw = (2.0 ** (np.arange(kcap) % 5)).astype(np.float32)
    da, db = dict(d), dict(d)
    da["wsnap"] = np.where(np.isnan(d["wsnap"]), np.float32(np.nan), pw[None, :]).astype(np.float32)
    db["wsnap"] = np.where(np.isnan(d["wsnap"]), np.float32(np.nan), np.float32(1)).astype(np.float32)
    ca, _ = _run_block(da, _upload(da))
    cb, _ = _run_block(db, _upload(db))
    n = 0
    for c, K in enumerate(Ks):
        a, b = ca[c, :, :K].astype(np.float64), cb[c, :, :K].astype(np.float64)
        ok = (np.abs(b) >= 2.0 ** -14) & np.isfinite(a)                               # normal float16 on both sides
        assert ok.mean() > 0.999
        assert np.array_equal(a[ok], (b * pw[None, :K].astype(np.float64))[ok])
        assert (_bits(ca[c, :, K:]) == 0).all() and (_bits(cb[c, :, K:]) == 0).all()
        n += int(ok.sum())
    assert n > 0.999 * TB * sum(Ks)


@gpu
def test_coefficients_are_standard_normal_draws():
    """wsnap = 1: C x TB x K = 2e5 coefficients are float16-rounded N(0, 1) draws (fixed seed): mean, variance and fourth moment
    within 5 standard errors; different steps, rows and chains are different draws."""
    Ks, kcap, p = (1043, 1043, 1043), 1043, 5
    d = _make(6, Ks, kcap, None, p, 8)
    d["wsnap"] = np.ones_like(d["wsnap"])
    coef, _ = _run_block(d, _upload(d))
    assert (_bits(coef[:, :, 1043:]) == 0).all()
    v = coef[:, :, :1043].astype(np.float64).ravel()
    n = v.size
    assert n > 2e5 and np.isfinite(v).all()
    assert abs(v.mean()) < 5 / np.sqrt(n)
    assert abs(v.var() - 1) < 5 * np.sqrt(2 / n)
    assert abs((v ** 4).mean() - 3) < 5 * np.sqrt(96 / n)
    cf = coef[:, :, :1043].astype(np.float64)
    assert abs(np.corrcoef(cf[0, 3], cf[0, 4])[0, 1]) < 0.2 and abs(np.corrcoef(cf[0, 3], cf[1, 3])[0, 1]) < 0.2
    assert abs(np.corrcoef(cf[0, :, 10], cf[0, :, 11])[0, 1]) < 0.6                   # (64 draws each)


# ------------------------------------------------------------------------------------------------------ 3. k_propose_hist
@gpu
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_single_step_matches_longdouble_reference(case):
    """out = cur + s_lr (sum coef hist / S - (sum coef) mean) + s_iso z with the block call's coefficients of the same absolute
    step and the step's elementwise normals; float64 fma accumulation: (K + 8) 2^-53 x the sum of the terms' magnitudes."""
    import torch
    _lib, L = _L()
    name, Ks, kcap, ksnap, p, pstride, use_hscale = case
    d = _make(1000 + CASES.index(case), Ks, kcap, ksnap, p, pstride, use_hscale)
    g = _upload(d)
    C, step0 = len(Ks), 23
    coef, _ = _run_block(d, g, step0=step0)
    ld = np.longdouble
    worst = (0.0, None)
    for t in (0, 29, TB - 1):
        s = step0 + t
        z = _normals(C, p, s)
        out = _nan_like((C, p))
        sp = _dev(np.array([s, -1], dtype=np.int64))
        _lib.check(L.qn_mcmc_propose_hist(g["cur"].data_ptr(), g["hist"].data_ptr(), g["wsnap"].data_ptr(), g["ksnap"].data_ptr(),
                                          g["mean"].data_ptr(), _ptr(g["hscale"]), S_LR, S_ISO, C, CHAIN0, p, pstride, kcap, SEED,
                                          sp.data_ptr(), out.data_ptr(), None), "propose_hist")
        torch.cuda.synchronize()
        out = out.cpu().numpy()
        for c, K in enumerate(Ks):
            cf = coef[c, t, :K].astype(ld)
            terms = cf[:, None] * d["hist"][c, :K, :p].astype(ld)
            m, cu, zi = d["mean"][c].astype(ld), d["cur"][c].astype(ld), ld(S_ISO) * z[c].astype(ld)
            Sc = ld(d["S"][c])
            ref = cu + ld(S_LR) * (terms.sum(axis=0) / Sc - cf.sum() * m) + zi
            mag = np.abs(cu) + ld(S_LR) * (np.abs(terms).sum(axis=0) / Sc + np.abs(cf).sum() * np.abs(m)) + np.abs(zi)
            bound = (K + 8) * ld(2.0) ** -53 * mag
            r, at = _worst(np.abs(out[c].astype(ld) - ref).astype(np.float64), bound.astype(np.float64))
            if r > worst[0]:
                worst = (r, (c, t) + at)
    print(f"\npropose_hist {name}: max err/bound = {worst[0]:.4g} at (chain, t, col) = {worst[1]}")
    assert worst[0] <= 1.0, (name, worst)


# ------------------------------------------------------------------------- 4. k_apply_delta, k_propose and k_accept loops
@gpu
@pytest.mark.parametrize("p", [1, 2, 513, 1031])
def test_apply_delta_matches_numpy(p):
    import torch
    _lib, L = _L()
    rs = np.random.RandomState(p)
    C, step = 3, 41
    cur, delta = 50.0 * rs.randn(C, p), 3.0 * rs.randn(C, TB, p)
    gc, gd = _dev(cur), _dev(delta)
    z = _normals(C, p, step)
    sp = _dev(np.array([step, -1], dtype=np.int64))
    worst = 0.0
    for t in (0, 7, TB - 1):
        out = _nan_like((C, p))
        _lib.check(L.qn_mcmc_apply_delta(gc.data_ptr(), gd.data_ptr(), t, S_ISO, C, CHAIN0, p, SEED, sp.data_ptr(), out.data_ptr(), None),
                   "apply_delta")
        torch.cuda.synchronize()
        ld = np.longdouble
        ref = cur.astype(ld) + delta[:, t].astype(ld) + ld(S_ISO) * z.astype(ld)
        bound = 2.0 ** -52 * (np.abs(cur + delta[:, t]) + np.abs(S_ISO * z))
        r, _ = _worst(np.abs(out.cpu().numpy().astype(ld) - ref).astype(np.float64), bound)
        worst = max(worst, r)
    print(f"\napply_delta p={p}: max err/bound = {worst:.4g}")
    assert worst <= 1.0


@gpu
def test_propose_grid_stride_second_pass():
    """k_propose caps its grid at 64 workgroups of 256 pairs: at p = 32768 + 5 the last pairs come from a second pass of its
    grid-stride loop.  Its normals equal, bit for bit, those k_apply_delta adds (one thread per pair, no loop)."""
    import torch
    _lib, L = _L()
    C, p, step = 2, 32768 + 5, 9
    z = _normals(C, p, step)
    assert np.isfinite(z).all()
    zero, dz = torch.zeros(C, p, dtype=torch.float64, device="cuda"), torch.zeros(C, TB, p, dtype=torch.float64, device="cuda")
    out = _nan_like((C, p))
    sp = _dev(np.array([step, -1], dtype=np.int64))
    _lib.check(L.qn_mcmc_apply_delta(zero.data_ptr(), dz.data_ptr(), 0, 1.0, C, CHAIN0, p, SEED, sp.data_ptr(), out.data_ptr(), None),
               "apply_delta")
    torch.cuda.synchronize()
    assert np.array_equal(_bits(z), _bits(out.cpu().numpy()))
    assert not np.array_equal(z[0, 32768:], z[0, :5]) and not np.array_equal(z[0], z[1])


@gpu
@pytest.mark.parametrize("p,par", [(65536 + 3, 0), (2 * 65536 + 6, 1)])
def test_accept_further_passes(p, par):
    """k_accept covers 65536 elements of a chain per pass of its grid (64 workgroups x 256 threads x 2 pairs): one direct step at
    sizes that need a second and a third pass.  Chain 0 accepts (current log-posterior -1e300), chain 1 rejects (SSE = inf);
    every input is a small dyadic number, so every operation is exact and everything is compared bit for bit."""
    import torch
    _lib, L = _L()
    rs = np.random.RandomState(p)
    C, kcap, nmcmc, step, S = 2, 4, 5, 3, 256.0
    pstride = _ceil4(p) + 4
    x0 = rs.randint(-512, 512, (C, p)) / 64.0
    cur_old = x0 + rs.randint(-2048, 2048, (C, p)) / 512.0
    dx = rs.randint(-4096, 4096, (C, p)) / 1024.0
    # (x - x0) S beyond +-65504 (saturation), at 65520 (rounds to inf without the clamp), in the first and the later passes
    for i, v in zip((0, 1, 2, 3, p - 1, p - 2, 65536, 65537, p // 2), (300.0, -300.0, 255.875, 255.9375, -255.9375, 257.0, -1000.0, 256.0, 511.0)):
        dx[:, i] = v
    prop = x0 + dx
    assert np.array_equal(prop - x0, dx)                                              # exact
    sumx_old = rs.randint(-64, 64, (C, p)) / 16.0
    mult_old = np.array([[3, 0, 0, 0], [2, 5, 4, 0]], dtype=np.int32)
    so, sn = par, 1 - par

    def slots(old, other, dtype):
        a = np.empty((2, C), dtype=dtype)
        a[so], a[sn] = old, other
        return a
    cur_lp = slots([-1e300, -1.0], np.nan, np.float64)
    best_lp = slots([-1e300, 5.0], np.nan, np.float64)
    kcur = slots([0, 2], -9, np.int32)
    step_ptr = np.empty(2, dtype=np.int64); step_ptr[so], step_ptr[sn] = step, -77
    sentinel = np.uint16(0x5A5A)
    hist0 = np.full((C, kcap, pstride), sentinel, dtype=np.uint16)
    g = dict(prop=_dev(prop), sse=_dev(np.array([[2.0], [np.inf]])), cur=_dev(cur_old), cur_lp=_dev(cur_lp),
             best=_dev(np.full((C, p), 7.5)), best_lp=_dev(best_lp), chain=_nan_like((C, nmcmc + 1, p)), lps=_nan_like((C, nmcmc + 1)),
             alphas=_nan_like((C, nmcmc + 1)), nacc=_dev(np.array([10, 20], dtype=np.int64)), x0=_dev(x0),
             hist=_dev(hist0.view(np.float16)), hscale=_dev(np.full(C, S)), mult=_dev(mult_old), kcur=_dev(kcur), sumx=_dev(sumx_old),
             step_ptr=_dev(step_ptr))
    # sigma = 1, n_rows = 0: log-posterior = -sse / 2 exactly
    _lib.check(L.qn_mcmc_accept(g["prop"].data_ptr(), g["sse"].data_ptr(), 1.0, 0, C, CHAIN0, p, nmcmc, SEED, g["cur"].data_ptr(),
                                g["cur_lp"].data_ptr(), g["best"].data_ptr(), g["best_lp"].data_ptr(), g["chain"].data_ptr(),
                                g["lps"].data_ptr(), g["alphas"].data_ptr(), g["nacc"].data_ptr(), g["x0"].data_ptr(),
                                g["hist"].data_ptr(), g["hscale"].data_ptr(), g["mult"].data_ptr(), g["kcur"].data_ptr(),
                                g["sumx"].data_ptr(), kcap, pstride, g["step_ptr"].data_ptr(), par, 1, None), "accept")
    torch.cuda.synchronize()
    r = {k: v.cpu().numpy() for k, v in g.items()}
    eq = lambda a, b: np.array_equal(_bits(a), _bits(np.asarray(b, dtype=a.dtype)))   # noqa: E731
    assert eq(r["cur"][0], prop[0]) and eq(r["cur"][1], cur_old[1])
    assert eq(r["best"][0], prop[0]) and eq(r["best"][1], np.full(p, 7.5))
    assert eq(r["chain"][0, step + 1], prop[0]) and eq(r["chain"][1, step + 1], cur_old[1])
    assert np.isnan(np.delete(r["chain"], step + 1, axis=1)).all()
    hist = r["hist"].view(np.uint16)
    want = np.clip(((prop[0] - x0[0]) * S).astype(np.float32), -65504.0, 65504.0).astype(np.float16)
    assert np.isfinite(want).all() and (np.abs(want.astype(np.float64)) == 65504.0).sum() >= 6
    assert np.array_equal(hist[0, 1, :p], _bits(want))
    assert (hist[0, 1, p:] == sentinel).all() and (hist[0, [0, 2, 3]] == sentinel).all() and (hist[1] == sentinel).all()
    assert eq(r["sumx"][0], sumx_old[0] + 3.0 * (cur_old[0] - x0[0])) and eq(r["sumx"][1], sumx_old[1])
    assert np.array_equal(r["mult"], [[3, 1, 0, 0], [2, 5, 5, 0]])
    assert np.array_equal(r["kcur"][sn], [1, 2]) and np.array_equal(r["kcur"][so], [0, 2])
    assert np.array_equal(r["nacc"], [11, 20])
    assert eq(r["cur_lp"][sn], [-1.0, -1.0]) and eq(r["cur_lp"][so], [-1e300, -1.0])
    assert eq(r["best_lp"][sn], [-1.0, 5.0]) and eq(r["best_lp"][so], [-1e300, 5.0])
    assert eq(r["lps"][:, step + 1], [-1.0, -1.0]) and np.isnan(np.delete(r["lps"], step + 1, axis=1)).all()
    assert eq(r["alphas"][:, step + 1], [np.inf, 0.0]) and np.isnan(np.delete(r["alphas"], step + 1, axis=1)).all()
    assert r["step_ptr"][so] == step and r["step_ptr"][sn] == step + 1


# -------------------------------------------------------------- self-check of the reference and the bound (no device needed)
def _host_coef(rs, d):
    """float16(wsnap x N(0, 1)) as k_hist_coef forms them, zero beyond K"""
    C, kcap = len(d["Ks"]), d["kcap"]
    coef = np.zeros((C, TB, _kstride(kcap)), dtype=np.float16)
    for c, K in enumerate(d["Ks"]):
        coef[c, :, :K] = (d["wsnap"][c, None, :K] * rs.randn(TB, K).astype(np.float32)).astype(np.float16)
    return coef


@pytest.mark.parametrize("Ks,kcap,p", [((1, 7, 15), 18, 5), ((16, 17, 40), 61, 130), ((127, 128, 129), 132, 130), ((136, 257, 300), 303, 130),
                                       ((40, 129, 300), 303, 1030)])
def test_bound_rejects_a_wrong_product(Ks, kcap, p):
    """The tests above bite: the reference recomputed with one history row dropped, two adjacent columns swapped, or the sum
    stopped at K - 1 misses the stated bound by more than 100 x at its worst element, for every chain at K <= 300.  The bound
    grows as K^2, one row's share does not: worst element 3e2-3e3 x at K = 300 (median over a chain's elements 30-60 x), 2e3 x
    at K = 128, 1e4-1e5 x at K <= 40; swapped columns 5e3 x and more.  The kernels' measured errors are 1e-4 .. 3e-2 of the bound
    (docs/experiments.md R5.2).  The unchanged reference in another summation order stays 10^6 x inside it."""
    rs = np.random.RandomState(p + sum(Ks))
    d = _make(p, Ks, kcap, None, p, _ceil4(p))
    coef = _host_coef(rs, d)
    ref, mag = block_reference(coef, d["hist"], d["mean"], d["S"], Ks, p, S_LR)
    bound = block_bound(ref, mag, Ks, S_LR)
    assert np.isfinite(ref).all() and (bound > 0).all()
    for c, K in enumerate(Ks):                                                        # float64 in reversed row order: the reference's own error
        cf, h = coef[c, :, :K].astype(np.float64)[:, ::-1], d["hist"][c, :K, :p].astype(np.float64)[::-1]
        alt = S_LR * (cf @ h / d["S"][c] - cf.sum(axis=1)[:, None] * d["mean"][c][None, :])
        assert (np.abs(alt - ref[c]) <= 1e-6 * bound[c]).all()
    muts = [("row dropped", dict(drop_row=3)), ("last row dropped", dict(stop_short=True))]
    muts += [("columns swapped", dict(swap_cols=j)) for j in sorted({0, p - 2, (p // 2) | 1} - {-1})]
    for what, kw in muts:
        bad, _ = block_reference(coef, d["hist"], d["mean"], d["S"], Ks, p, S_LR, **kw)
        for c in range(len(Ks)):
            r = (np.abs(bad[c] - ref[c]) / bound[c]).max()
            assert r > 100.0, (what, kw, c, r)


def test_bound_at_the_longest_history():
    """K = 4100 (33 chunks of 128 rows): the float32 bound is (K + 16) 2^-23 = 5e-4 of the sum of K magnitudes, so one dropped row
    of 4100 exceeds it only by 1.7 x at the worst element (6-10 x at K = 2047 / 2048), a dropped 128-row chunk by 16-70 x, swapped
    columns by 100-450 x.  Single rows are pinned at the shorter histories above; what this length adds for the block kernel is
    the chunk count.  (The single-step kernel's float64 bound at the same shape is 2^29 times tighter.)"""
    Ks, kcap, p = (2047, 2048, 4100), 4103, 5
    rs = np.random.RandomState(11)
    d = _make(12, Ks, kcap, None, p, 8)
    coef = _host_coef(rs, d)
    ref, mag = block_reference(coef, d["hist"], d["mean"], d["S"], Ks, p, S_LR)
    bound = block_bound(ref, mag, Ks, S_LR)
    for what, kw, least in (("row dropped", dict(drop_row=3), 1.0), ("last row dropped", dict(stop_short=True), 1.0),
                            ("chunk dropped", dict(drop_chunk=15), 10.0), ("columns swapped", dict(swap_cols=2), 10.0)):
        bad, _ = block_reference(coef, d["hist"], d["mean"], d["S"], Ks, p, S_LR, **kw)
        for c in range(len(Ks)):
            r = (np.abs(bad[c] - ref[c]) / bound[c]).max()
            assert r > least, (what, c, r)
