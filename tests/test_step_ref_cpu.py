"""A host model of the two kernels every device sampler keeps its state through -- the Metropolis-Hastings accept step
(`k_accept`, csrc/qn_mcmc.hip) and the whitened leapfrog (`k_hmc_begin` / `k_hmc_leap`, csrc/qn_hmc_leap.hip) -- written from
include/quinn_amd.h and the kernels' comments in plain numpy, the inputs of the direct device tests of
tests/test_gpu_step_kernels.py, and the checks of both that need no device.

The model is exact, not approximate: with the inputs used here (sigma = 1 and n_rows = 0, so log-posterior = -SSE / 2; small
dyadic numbers; power-of-two factors) every product the kernels form is exact, so a fused multiply-add and numpy's multiply +
add round the same sum once, and everything but exp() can be held bit for bit.  The functions below say where that matters.

`mutate=` recomputes a step WRONG on purpose: the self-checks at the end show that the inputs of the device tests tell every
listed wrong variant from the right one."""
import math

import numpy as np
import pytest

from quinn_amd.mcmc.ess import u01
from quinn_amd.mcmc.sgmcmc import ctr_of, philox4x32

LD = np.longdouble
SEED, SEED2, CHAIN0 = 1234, 987654321, 5
HIST_SENTINEL = np.uint16(0x5A5A)
MUTATIONS = ("stream", "le", "gt", "parts64", "kin_short", "beta_nlp", "gcur_always")       # of accept_np; the leapfrog's: parts_touched


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same(a, b):
    """equal bit for bit; two NaN count as equal whatever their payload (a device exp(NaN) against numpy's)"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    eq = bits(a) == bits(b)
    if a.dtype.kind == "f":
        eq = eq | (np.isnan(a) & np.isnan(b))
    return bool(eq.all())


def ulps(got, ref):
    """distance of the float64 `got` from the longdouble `ref` in units of the last place of ref"""
    ref = np.asarray(ref, dtype=LD)
    return np.abs(np.asarray(got).astype(LD) - ref) / np.spacing(np.abs(ref.astype(np.float64))).astype(LD)


def lsum(v):
    """float64 sum, left to right, from 0"""
    s = np.float64(0.0)
    for x in np.asarray(v, dtype=np.float64).ravel():
        s = s + x
    return s


def accept_uniform(seed, step, chain, stream_offset=1):
    """the accept uniform of GLOBAL chain `chain` at `step`: words 0, 1 of the block (seed, 2 step + 1, [chain][2][0])"""
    w = philox4x32(seed, 2 * int(step) + stream_offset, ctr_of(int(chain), 2, 0))
    return np.float64(u01(w[0], w[1]))


def hist_row(x, x0, S):
    """float16(clip((x - x0) S, +-65504)), through float32 as the device converts"""
    return np.clip(((x - x0) * S).astype(np.float32), -65504.0, 65504.0).astype(np.float16)


def new_state(cur, cur_lp, best_lp, step, par, nmcmc, best=None, nacc=None, chain=True, grad_cur=None, hist=None):
    """The state one accept call works on.  The double-buffered scalars hold the given values in slot `par` and NaN / -9 / -77
    in the slot the call must write; chain / lps / alphas are NaN.  hist: dict(x0, kcap, pstride, hscale or None, mult, kcur,
    sumx): rows filled with HIST_SENTINEL."""
    cur = np.array(cur, dtype=np.float64)
    C, p = cur.shape

    def slots(old, other, dtype):
        a = np.empty((2, C), dtype=dtype)
        a[par], a[1 - par] = old, other
        return a
    st = dict(cur=cur, cur_lp=slots(cur_lp, np.nan, np.float64), best_lp=slots(best_lp, np.nan, np.float64),
              best=np.full((C, p), 7.5) if best is None else np.array(best, dtype=np.float64),
              lps=np.full((C, nmcmc + 1), np.nan), alphas=np.full((C, nmcmc + 1), np.nan),
              nacc=np.zeros(C, dtype=np.int64) if nacc is None else np.array(nacc, dtype=np.int64),
              step_ptr=np.empty(2, dtype=np.int64))
    st["step_ptr"][par], st["step_ptr"][1 - par] = step, -77
    if chain:
        st["chain"] = np.full((C, nmcmc + 1, p), np.nan)
    if grad_cur is not None:
        st["grad_cur"] = np.array(grad_cur, dtype=np.float64)
    if hist is not None:
        kcap, pstride = hist["kcap"], hist["pstride"]
        st["x0"] = np.array(hist["x0"], dtype=np.float64)
        st["hist"] = np.full((C, kcap, pstride), HIST_SENTINEL, dtype=np.uint16).view(np.float16)
        st["hscale"] = None if hist.get("hscale") is None else np.array(hist["hscale"], dtype=np.float64)
        st["mult"] = np.array(hist["mult"], dtype=np.int32)
        st["kcur"] = slots(hist["kcur"], -9, np.int32)
        st["sumx"] = np.array(hist["sumx"], dtype=np.float64)
    return st


def accept_np(state, prop, sse_parts, sigma, n_rows, chain0, seed, par, kin_cur=None, kin_prop=None, gprop=None, beta=None,
              hist=None, mutate=None):
    """One accept step of all chains -> the new state (the old one is left alone).  Slot `par` of cur_lp / best_lp / kcur /
    step_ptr is read, slot 1 - par written.

        sse = sum of the chain's SSE parts, left to right;  plp = -(0.5 / sigma^2 * sse + lp_const)
        mh  = exp((-(beta clp) + K_cur / 2) - (-(beta plp) + K_prop / 2)),  K = the chain's kinetic parts, left to right
        accept iff u < mh (strict; NaN rejects), u = accept_uniform(seed, step, chain0 + b)
        accepted: cur <- prop, grad_cur <- gprop, nacc += 1, and best / best_lp <- the proposal when plp >= best_lp
        lps[b, step + 1] = the (untempered) log-posterior of the new state, alphas[b, step + 1] = mh, chain[b, step + 1] = cur
        step_ptr[1 - par] = step + 1
    History (state has 'hist'): row k of a chain is float16((x_k - x0) S) of its k-th distinct state, mult[k] the length of
    the stay there, kcur the row of the current state; sumx collects mult x (x - x0) of a state when the chain LEAVES it.
    A full history (row index >= kcap) takes no row, no multiplicity and no sum any more; kcur goes on counting.
    alphas come from numpy's exp here: the device's may differ in the last places (tests hold it to 4 ulp of a longdouble exp)
    unless mh is 0, inf or NaN."""
    st = state
    new = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in st.items()}
    prop = np.asarray(prop, dtype=np.float64)
    C, p = st["cur"].shape
    so, sn = par, 1 - par
    step = int(st["step_ptr"][so])
    with_hist = ("hist" in st) if hist is None else hist
    half_inv_sig2 = 0.5 / (sigma * sigma)
    lp_const = 0.5 * n_rows * math.log(2.0 * math.pi) + n_rows * math.log(sigma)
    sse_parts = np.asarray(sse_parts, dtype=np.float64).reshape(C, -1)
    with np.errstate(all="ignore"):
        for b in range(C):
            sse = lsum(sse_parts[b, :64] if mutate == "parts64" else sse_parts[b])
            plp = -(half_inv_sig2 * sse + lp_const)
            clp, blp = st["cur_lp"][so, b], st["best_lp"][so, b]
            bc = np.float64(1.0 if beta is None else beta[b])
            k_c = lsum(kin_cur[b]) if kin_cur is not None else np.float64(0.0)
            k_p = np.float64(0.0)
            if kin_prop is not None:
                k_p = lsum(kin_prop[b][:-1] if mutate == "kin_short" else kin_prop[b])
            mh = np.exp((-(bc * clp) + 0.5 * k_c) - (-(bc * plp) + 0.5 * k_p))
            u = accept_uniform(seed, step, chain0 + b, 0 if mutate == "stream" else 1)
            take = bool(u <= mh) if mutate == "le" else bool(u < mh)
            nlp = plp if take else clp
            if mutate == "beta_nlp":
                nlp = bc * nlp
            better = take and bool(nlp > blp if mutate == "gt" else nlp >= blp)
            if with_hist:
                kcap = st["mult"].shape[1]
                kc = int(st["kcur"][so, b])
                knew = kc + 1 if take else kc
                new["kcur"][sn, b] = knew
                if take:
                    if kc < kcap:                                     # the stay the chain leaves (products exact: dyadic inputs)
                        new["sumx"][b] = st["sumx"][b] + np.float64(st["mult"][b, kc]) * (st["cur"][b] - st["x0"][b])
                    if knew < kcap:
                        S = 1.0 if st["hscale"] is None else st["hscale"][b]
                        new["hist"][b, knew, :p] = hist_row(prop[b], st["x0"][b], S)
                        new["mult"][b, knew] = 1
                elif kc < kcap:
                    new["mult"][b, kc] += 1
            if take:
                new["cur"][b] = prop[b]
                new["nacc"][b] += 1
            if "grad_cur" in st and gprop is not None and (take or mutate == "gcur_always"):
                new["grad_cur"][b] = gprop[b]
            if better:
                new["best"][b] = prop[b]
            new["cur_lp"][sn, b] = nlp
            new["best_lp"][sn, b] = nlp if better else blp
            new["lps"][b, step + 1] = nlp
            new["alphas"][b, step + 1] = mh
            if st.get("chain") is not None:
                new["chain"][b, step + 1] = new["cur"][b]
    new["step_ptr"][sn] = step + 1
    return new


# ------------------------------------------------------------------------------------------------------------- leapfrog
def hmc_parts(p):
    """qn_hmc_parts: workgroups (= kinetic partial sums) per chain"""
    return min(64, max(1, -(-p // 1024)))


def part_ranges(p, pairs):
    """[lo, hi) in ELEMENTS of every partial sum: n = p elements (leap) or ceil(p / 2) pairs (begin) in chunks of ceil(n / parts)"""
    parts = hmc_parts(p)
    n = (p + 1) // 2 if pairs else p
    chunk = -(-n // parts)
    out = []
    for k in range(parts):
        lo, hi = min(k * chunk, n), min((k + 1) * chunk, n)
        out.append((min(2 * lo, p), min(2 * hi, p)) if pairs else (lo, hi))
    return out


def _per_chain(v, C, ft):
    return np.broadcast_to(np.asarray(v, dtype=ft), (C,)).reshape(C, 1)


def fixed_order_sum_of_squares(z, lo, hi):
    """sum z[lo:hi]^2 in the fixed order of the begin kernel's workgroup (lo even): thread t of 256 takes the pairs t, t + 256, ...
    of the range and adds their squares in turn, the first element of a pair before the second; the 64 threads of a wave are
    folded by halving (i += i + 32, 16, .. 1); the four waves as (w0 + w1) + (w2 + w3).  z has 24-bit significands, so each
    square is exact and only the additions round: float64 numpy reproduces the sum bit for bit."""
    n = hi - lo
    npair = (n + 1) // 2
    trips = max(1, -(-npair // 256))
    sq = np.zeros(trips * 512)
    sq[:n] = np.square(z[lo:hi])
    sq = sq.reshape(trips, 256, 2)
    acc = np.zeros(256)
    for r in range(trips):
        acc = acc + sq[r, :, 0]
        acc = acc + sq[r, :, 1]
    red = []
    for w in range(4):
        x = acc[64 * w:64 * w + 64]
        for off in (32, 16, 8, 4, 2, 1):
            x = x[:off] + x[off:2 * off]
        red.append(x[0])
    return (red[0] + red[1]) + (red[2] + red[3])


def begin_np(cur, gcur, z, sigma, eps, scale=None, beta=None, ft=np.float64):
    """Start of a trajectory for the momentum draw z [C, p]:  mom = z + (hk_c s) g_cur,  q = cur + (eps_c s) mom,
    hk_c = (eps_c / 2) gs beta_c, gs = -0.5 / sigma^2;  K_cur parts [C, parts] = sums of z^2 over the chunks of PAIRS.
    -> mom, q, kin_parts.  Each sum is rounded once, as the kernel's fma does, PROVIDED its product is exact (products_exact)."""
    C, p = cur.shape
    e, b_ = _per_chain(eps, C, ft), _per_chain(1.0 if beta is None else beta, C, ft)
    s = ft(1.0) if scale is None else np.asarray(scale, dtype=ft)
    gs = ft(-0.5) / (ft(sigma) * ft(sigma)) * b_
    hk = ft(0.5) * e * gs
    mom = z.astype(ft) + (hk * s) * gcur.astype(ft)
    q = cur.astype(ft) + (e * s) * mom
    kin = np.array([[fixed_order_sum_of_squares(z[c], lo, hi) for lo, hi in part_ranges(p, True)] for c in range(C)])
    return mom, q, kin


def parts_touched(p, k, wrong=False):
    """elements that enter partial sum k of the leap kernel.  wrong: a workgroup of 256 threads x 4 elements per trip that
    bounds its elements by p in place of its chunk's end -- the last trip of a chunk runs on into the next chunk"""
    lo, hi = part_ranges(p, False)[k]
    if not wrong:
        return np.arange(lo, hi)
    out = []
    for e0 in range(lo, hi, 1024):
        t = np.arange(e0, min(e0 + 256, hi))
        out.append(np.concatenate([t + 256 * u for u in range(4)]))
    e = np.concatenate(out) if out else np.arange(0)
    return np.sort(e[e < p])


def leap_np(g, mom, q, sigma, eps, last, scale=None, beta=None, ft=np.float64, mutate=None):
    """One leapfrog call:  mom += (kick_c s) g, kick_c = f eps_c gs beta_c, f = 1/2 on the last call and 1 before;
    inner call: q += (eps_c s) mom, no kinetic parts;  last call: q as it was, K_prop parts [C, parts] = sums of mom^2 over the
    chunks of elements.  -> mom, q, kin_parts (None on an inner call)"""
    C, p = mom.shape
    e, b_ = _per_chain(eps, C, ft), _per_chain(1.0 if beta is None else beta, C, ft)
    s = ft(1.0) if scale is None else np.asarray(scale, dtype=ft)
    gs = ft(-0.5) / (ft(sigma) * ft(sigma)) * b_
    kick = ft(0.5 if last else 1.0) * e * gs
    m = mom.astype(ft) + (kick * s) * g.astype(ft)
    if not last:
        return m, q.astype(ft) + (e * s) * m, None
    m2 = np.square(m)
    kin = np.array([[m2[c, parts_touched(p, k, mutate == "parts_touched")].sum() for k in range(hmc_parts(p))] for c in range(C)])
    return m, q.astype(ft), kin


def products_exact(*pairs):
    """every elementwise product a * b of the pairs is exact in float64 (its 64-bit longdouble value is a float64)"""
    for a, b in pairs:
        a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
        if not np.array_equal(a.astype(LD) * b.astype(LD), (a * b).astype(LD)):
            return False
    return True


def leap_factors(sigma, eps, last, scale, beta, C):
    """(kick_c s, eps_c s) as float64 arrays, and whether the scalar products behind them are exact"""
    e, b_ = _per_chain(eps, C, np.float64), _per_chain(1.0 if beta is None else beta, C, np.float64)
    s = np.float64(1.0) if scale is None else np.asarray(scale, dtype=np.float64)
    gs0 = -0.5 / (sigma * sigma)
    f = 0.5 if last else 1.0
    ok = products_exact((gs0, b_), (f, e), (f * e, gs0 * b_), (f * e * (gs0 * b_), s), (e, s))
    return (f * e * (gs0 * b_)) * s, e * s, ok


# -------------------------------------------------------------------------------- inputs of the device tests (and of the checks below)
def dyadic(rs, shape, den=8, lim=8):
    """multiples of 1 / den in (-lim, lim)"""
    return rs.randint(-den * lim + 1, den * lim, shape) / float(den)


def threshold_sse(seed, chain0, C, step, first=0):
    """SSE [C, 1] that puts chain b's mh = exp(-sse / 2) at u_b (1 + s 2^-40), s = +1 for even first + b (accept), -1 for odd
    (reject).  log, the multiply and the device's exp err by a few 2^-53 together; the margin is 2^13 times that, and any
    other uniform still flips about half the chains."""
    u = np.array([accept_uniform(seed, step, chain0 + b) for b in range(C)])
    s = np.where((first + np.arange(C)) % 2 == 0, 1.0, -1.0)
    return (-2.0 * np.log(u * (1.0 + s * 2.0 ** -40))).reshape(C, 1), u, s > 0


def threshold_state(C, p, step, par, nmcmc=4, with_grad=False):
    rs = np.random.RandomState(100 + step)
    return new_state(dyadic(rs, (C, p)), np.zeros(C), np.zeros(C), step, par, nmcmc, grad_cur=dyadic(rs, (C, p)) if with_grad else None)


SPECIAL = ("sse nan", "sse inf", "clp -inf", "both -inf", "tie with best", "below best")


def special_case(par=1, step=1):
    """-> state, prop, sse [6, 1], expected (take, alpha) per chain; sigma = 1, n_rows = 0"""
    rs = np.random.RandomState(7)
    C, p = len(SPECIAL), 3
    clp = np.array([-1.0, -1.0, -np.inf, -np.inf, -1e300, -1e300])
    blp = np.array([5.0, 5.0, -np.inf, -np.inf, -1.0, 5.0])
    sse = np.array([np.nan, np.inf, 2.0, np.inf, 2.0, 2.0]).reshape(C, 1)
    st = new_state(dyadic(rs, (C, p)), clp, blp, step, par, 3)
    want = [(False, np.nan), (False, 0.0), (True, np.inf), (False, np.nan), (True, np.inf), (True, np.inf)]
    return st, dyadic(rs, (C, p)), sse, want


NPARTS = (1, 2, 63, 64, 65, 130)


def parts_case(nparts):
    """SSE parts [2, nparts] whose float64 sum depends on the order: large terms that cancel between small ones (the pattern
    [2^k, a, -2^k, b] with k and the small terms varying), so every part counts.  Both chains accept (cur_lp = -1e300)."""
    rs = np.random.RandomState(nparts)
    C = 2
    big = 2.0 ** rs.randint(53, 57, (C, nparts)) * (1 + rs.randint(0, 8, (C, nparts)) / 8.0)
    small = rs.randint(1, 2 ** 24, (C, nparts)) / 16.0               # loses its last places beside a large term, never all of itself
    i = np.arange(nparts)
    parts = np.where(i % 4 == 0, big, np.where(i % 4 == 2, -np.roll(big, 2, axis=1), small))
    if nparts <= 2:
        parts = small + np.where(i == 0, big, 0.0)
    st = new_state(dyadic(rs, (C, 3)), np.full(C, -1e300), np.full(C, -1e300), 2, 0, 4)
    return st, dyadic(rs, (C, 3)), parts


HMC_P = (1, 2, 1023, 1025, 4353, 65537)
HMC_BETA = (1.0, 0.5, 0.25)
HMC_TARGET = np.array([3.0, -40.0, -0.25])             # the exponent's argument per chain: accept, reject, decided by u


def hmc_case(p, beta, par=1, step=2):
    """C = 3 chains of odd / even length p with nkin = hmc_parts(p) kinetic parts each, all different small dyadics; SSE chosen so
    that the argument of exp is HMC_TARGET exactly.  -> state, q, grad_q, sse [3, 1], kin_cur, kin_prop, beta [3]"""
    rs = np.random.RandomState(p)
    C, nk = 3, hmc_parts(p)
    i, b = np.arange(nk)[None, :], np.arange(C)[:, None]
    kin_cur = (i + 1 + b) / 64.0
    kin_prop = (2 * i + 1 + b) / 128.0
    clp = np.array([-512.0, -513.0, -514.5])
    a0 = (kin_cur.sum(axis=1) - kin_prop.sum(axis=1)) / 2
    plp = clp + (HMC_TARGET - a0) / beta
    sse = (-2.0 * plp).reshape(C, 1)
    st = new_state(dyadic(rs, (C, p)), clp, [-1e300, 0.0, 0.0], step, par, 4, grad_cur=dyadic(rs, (C, p)), nacc=[3, 4, 5])
    return st, dyadic(rs, (C, p)), dyadic(rs, (C, p)), sse, kin_cur, kin_prop, np.full(C, beta)


SIX_PATTERN = ("ARRAAA", "RARRAR", "AAARRA")


def six_step_case():
    """C = 3, p = 5, pstride = 12, kcap = 3, S = 256: six proposals [6, C, p] and SSE [6, C, 1] that force SIX_PATTERN --
    a reject by SSE = inf (mh = 0), an accept by a log-posterior 1024 above the current one (mh = exp(1024) = inf; the first
    from -1e300), so every alpha is exact.  Chains 0 and 2 fill their three rows and accept again afterwards."""
    rs = np.random.RandomState(66)
    C, p, kcap, pstride, S, nsteps = 3, 5, 3, 12, 256.0, 6
    x0 = dyadic(rs, (C, p), 64)
    dx = dyadic(rs, (nsteps, C, p), 1024, 4)
    dx[0, 0, 0], dx[3, 0, 1], dx[1, 2, 4] = 300.0, -257.0, 255.9375                 # (x - x0) S beyond / at the float16 limit
    props = x0[None] + dx
    assert np.array_equal(props - x0[None], dx)
    sse = np.empty((nsteps, C, 1))
    lp = np.full(C, -4096.0 * 8)
    for t in range(nsteps):
        for c in range(C):
            if SIX_PATTERN[c][t] == "A":
                lp[c] += 1024.0
                sse[t, c, 0] = -2.0 * lp[c]
            else:
                sse[t, c, 0] = np.inf
    hist = dict(x0=x0, kcap=kcap, pstride=pstride, hscale=np.full(C, S), mult=[[1, -5, -5]] * C, kcur=[0] * C, sumx=np.zeros((C, p)))
    st = new_state(x0 + dyadic(rs, (C, p), 512, 4), np.full(C, -1e300), np.full(C, -1e300), 0, 0, nsteps, hist=hist)
    return st, props, sse


LEAP_P = (1, 2, 1025, 65536, 65537, 70001, 200003)
LEAP_VARIANTS = ("fixed", "s", "s_noscale", "t", "t_noscale")


def leap_case(p, variant, for_begin):
    """C = 2; sigma in {0.5, 1} (gs = -2, -0.5).  begin: eps, scale, beta powers of two, so their products with the 53-bit
    mom = z + .. are exact; leap: small dyadics with more than one bit.  Gradients, momenta and positions multiples of 1/8 in
    (-8, 8).  -> dict(sigma, eps (float or [C]), scale, beta, g, mom, q)"""
    rs = np.random.RandomState(p % 100003 + 17 * LEAP_VARIANTS.index(variant) + (1 if for_begin else 0))
    C = 2
    d = dict(sigma=0.5 if LEAP_VARIANTS.index(variant) % 2 == 0 else 1.0, scale=None, beta=None)
    if variant == "fixed":
        d["eps"] = 0.25 if for_begin else 0.375
    else:
        d["eps"] = np.array([0.25, 0.5]) if for_begin else np.array([0.375, 0.5])
    if variant in ("s", "t"):
        d["scale"] = rs.choice([0.5, 1.0, 2.0] if for_begin else [0.5, 0.75, 1.25, 2.0], (C, p))
    if variant in ("t", "t_noscale"):
        d["beta"] = np.array([0.5, 0.25])
    d["g"], d["mom"], d["q"] = dyadic(rs, (C, p)), dyadic(rs, (C, p)), dyadic(rs, (C, p))
    return d


def fake_normals(rs, shape):
    """stand-ins for the device's momentum draws on the host: float32 normals (24-bit significands)"""
    return rs.randn(*shape).astype(np.float32).astype(np.float64)


# ================================================================================================ checks that need no device
def test_uniform_is_in_the_open_interval_and_keyed():
    u = np.array([[accept_uniform(SEED, s, c) for c in range(64)] for s in range(16)])
    assert ((u > 0) & (u < 1)).all() and np.unique(u).size == u.size
    assert np.array_equal(u, np.array([[accept_uniform(SEED, s, c) for c in range(64)] for s in range(16)]))
    assert abs(u.mean() - 0.5) < 5 / np.sqrt(12 * u.size)
    assert accept_uniform(SEED, 3, 7) != accept_uniform(SEED2, 3, 7)
    assert accept_uniform(SEED, 3, 7) != accept_uniform(SEED, 3, 7, stream_offset=0)
    w = philox4x32(SEED, 7, ctr_of(7, 1, 0))                                         # purpose 1: the scalar normal's block
    assert accept_uniform(SEED, 3, 7) != u01(w[0], w[1])


@pytest.mark.parametrize("kcap", [64, 4])
def test_bookkeeping_equals_a_recount_from_the_stored_chain(kcap):
    """40 steps with real decisions (mh around 1/2): multiplicities, distinct states, rows and the lazy sum against a recount
    from the stored chain.  kcap = 4: the history fills early; kcur goes on counting, rows, multiplicities and sum stop."""
    rs = np.random.RandomState(kcap)
    C, p, n, S = 4, 5, 40, 64.0
    x0 = dyadic(rs, (C, p), 64)
    hist = dict(x0=x0, kcap=kcap, pstride=8, hscale=np.full(C, S), mult=[[1] + [0] * (kcap - 1)] * C, kcur=[0] * C, sumx=np.zeros((C, p)))
    st = new_state(x0.copy(), np.full(C, -3.0), np.full(C, -3.0), 0, 0, n, hist=hist)
    st["chain"][:, 0] = x0
    for t in range(n):
        prop = x0 + dyadic(rs, (C, p), 256, 4)
        st = accept_np(st, prop, rs.uniform(4.0, 9.0, (C, 1)), 1.0, 0, CHAIN0, SEED, t & 1)
    so = n & 1
    assert st["step_ptr"][so] == n and not np.isnan(st["chain"]).any()
    rates = []
    for c in range(C):
        ch = st["chain"][c]
        starts = [0] + [i for i in range(1, n + 1) if not np.array_equal(ch[i], ch[i - 1])]
        runs = np.diff(starts + [n + 1])
        K = len(starts) - 1
        rates.append(K / n)
        assert st["kcur"][so, c] == K and st["nacc"][c] == K
        assert np.array_equal(st["cur"][c], ch[n])
        if K < kcap:
            assert np.array_equal(st["mult"][c, :K + 1], runs) and (st["mult"][c, K + 1:] == 0).all()
            total = (ch - x0[c]).sum(axis=0)                                         # dyadic: exact in any order
            assert np.array_equal(total, st["sumx"][c] + st["mult"][c, K] * (st["cur"][c] - x0[c]))
        else:                                                                        # full: stays of the rows < kcap that were LEFT while a row existed
            assert np.array_equal(st["mult"][c], runs[:kcap])
            assert np.array_equal(st["sumx"][c], sum(runs[k] * (ch[starts[k]] - x0[c]) for k in range(kcap)))
        for k in range(min(K + 1, kcap)):
            if k > 0:
                assert same(st["hist"][c, k, :p], hist_row(ch[starts[k]], x0[c], S))
        assert (bits(st["hist"][c, :, p:]) == HIST_SENTINEL).all() and (bits(st["hist"][c, min(K + 1, kcap):]) == HIST_SENTINEL).all()
        lp = st["lps"][c, 1:]
        assert same(st["cur_lp"][so, c], lp[-1]) and st["best_lp"][so, c] == max(-3.0, lp.max())
    assert 0.1 < np.mean(rates) < 0.9
    if kcap == 4:
        assert max(st["kcur"][so]) > kcap


def _take(st, step):
    return ~np.isnan(st["alphas"][:, step + 1]) & (st["nacc"] > 0)


def test_threshold_inputs_decide_as_stated_and_see_another_uniform():
    flips = 0
    for seed in (SEED, SEED2):
        for step in (0, 3):
            sse, u, acc = threshold_sse(seed, CHAIN0, 8, step)
            assert (sse > 0).all() and np.isfinite(sse).all()
            st = threshold_state(8, 3, step, step & 1)
            r = accept_np(st, st["cur"] + 1.0, sse, 1.0, 0, CHAIN0, seed, step & 1)
            assert np.array_equal(r["nacc"], acc.astype(np.int64))
            assert (ulps(r["alphas"][:, step + 1], np.exp((-0.5 * sse[:, 0]).astype(LD))) <= 4).all()
            assert not same(threshold_sse(seed, 0, 8, step)[0], sse)                 # the global chain id counts
            bad = accept_np(st, st["cur"] + 1.0, sse, 1.0, 0, CHAIN0, seed, step & 1, mutate="stream")
            flips += int((bad["nacc"] != r["nacc"]).sum())
            assert same(accept_np(st, st["cur"] + 1.0, sse, 1.0, 0, CHAIN0, seed, step & 1, mutate="le")["nacc"], r["nacc"])
    assert 8 <= flips <= 24                                                          # about half of 32


def tie_candidates(seed, chain_ids, step, width):
    """a chain whose uniform lies in (0.61, 0.77) -- there x = log u has a finer grid than u, so some x near log u has exp(x) == u
    -- and the SSE -2 x of the 2 width + 1 doubles x around log u.  -> chain id, u, sse [2 width + 1]"""
    for c in chain_ids:
        u = accept_uniform(seed, step, c)
        if 0.61 < u < 0.77:
            x = np.log(u)
            xs = x + np.arange(-width, width + 1) * np.spacing(x)
            return c, u, -2.0 * xs
    raise AssertionError("no uniform in (0.61, 0.77)")


def test_a_tie_rejects():
    """u < mh is strict: with mh == u the chain stays.  The only inputs on which `u <= mh` differs."""
    c, u, sse = tie_candidates(SEED, range(64), 1, 32)
    mh = np.exp(-0.5 * sse)
    assert (np.diff(mh) <= 0).all() and mh[0] > u > mh[-1]
    ties = np.flatnonzero(mh == u)
    assert ties.size >= 1
    for i in (ties[0], ties[0] - 8, ties[0] + 8):
        st = threshold_state(1, 3, 1, 1)
        r = accept_np(st, st["cur"] + 1.0, sse[i:i + 1], 1.0, 0, c, SEED, 1)
        bad = accept_np(st, st["cur"] + 1.0, sse[i:i + 1], 1.0, 0, c, SEED, 1, mutate="le")
        assert r["nacc"][0] == int(u < mh[i]) and (bad["nacc"][0] != r["nacc"][0]) == (i == ties[0])


def test_special_values_follow_the_rules():
    st, prop, sse, want = special_case()
    r = accept_np(st, prop, sse, 1.0, 0, CHAIN0, SEED, 1)
    for b, (take, alpha) in enumerate(want):
        assert r["nacc"][b] == int(take), SPECIAL[b]
        assert same(r["alphas"][b, 2], np.float64(alpha)), SPECIAL[b]
    assert same(r["best"][4], prop[4]) and r["best_lp"][0, 4] == -1.0 and same(r["best"][5], st["best"][5]) and r["best_lp"][0, 5] == 5.0
    bad = accept_np(st, prop, sse, 1.0, 0, CHAIN0, SEED, 1, mutate="gt")
    assert not same(bad["best"], r["best"]) and same(bad["best"][[0, 1, 2, 3, 5]], r["best"][[0, 1, 2, 3, 5]])


@pytest.mark.parametrize("nparts", NPARTS)
def test_parts_inputs_depend_on_the_order(nparts):
    st, prop, parts = parts_case(nparts)
    r = accept_np(st, prop, parts, 1.0, 0, CHAIN0, SEED, 0)
    assert np.isfinite(r["lps"][:, 3]).all() and (r["nacc"] == 1).all()
    for c in range(2):
        assert r["lps"][c, 3] == -0.5 * lsum(parts[c])
        if nparts > 2:                                                               # (one or two terms have one order)
            assert np.sum(parts[c]) != lsum(parts[c]) and lsum(parts[c][::-1]) != lsum(parts[c])
        for drop in range(nparts):                                                   # every part counts
            assert lsum(np.delete(parts[c], drop)) != lsum(parts[c])
    bad = accept_np(st, prop, parts, 1.0, 0, CHAIN0, SEED, 0, mutate="parts64")
    assert same(bad["lps"], r["lps"]) == (nparts <= 64)


@pytest.mark.parametrize("p", HMC_P)
@pytest.mark.parametrize("beta", HMC_BETA)
def test_hmc_inputs_are_exact_and_see_the_wrong_variants(p, beta):
    st, q, gq, sse, kc, kp, bt = hmc_case(p, beta)
    kw = dict(kin_cur=kc, kin_prop=kp, gprop=gq, beta=bt)
    r = accept_np(st, q, sse, 1.0, 0, CHAIN0, SEED, 1, **kw)
    arg = (-(LD(beta) * st["cur_lp"][1].astype(LD)) + kc.astype(LD).sum(axis=1) / 2) - \
          (-(LD(beta) * (-0.5 * sse[:, 0]).astype(LD)) + kp.astype(LD).sum(axis=1) / 2)
    assert np.array_equal(arg, HMC_TARGET.astype(LD))                                # exact
    assert (ulps(r["alphas"][:, 3], np.exp(HMC_TARGET.astype(LD))) <= 4).all()
    assert r["nacc"][0] == 4 and r["nacc"][1] == 4                                   # chain 0 accepts, chain 1 rejects
    assert same(r["grad_cur"][0], gq[0]) and same(r["grad_cur"][1], st["grad_cur"][1])
    assert same(r["lps"][0, 3], np.float64(-0.5 * sse[0, 0])) and same(r["lps"][1, 3], st["cur_lp"][1, 1])
    for m in ("kin_short", "gcur_always") + (("beta_nlp",) if beta != 1.0 else ()):
        bad = accept_np(st, q, sse, 1.0, 0, CHAIN0, SEED, 1, mutate=m, **kw)
        what = {"kin_short": "alphas", "gcur_always": "grad_cur", "beta_nlp": "lps"}[m]
        assert not same(bad[what], r[what]), m
        if m == "kin_short":
            assert (ulps(bad["alphas"][:, 3], np.exp(HMC_TARGET.astype(LD))) > 1e6).all()
    if beta == 1.0:
        assert same(accept_np(st, q, sse, 1.0, 0, CHAIN0, SEED, 1, kin_cur=kc, kin_prop=kp, gprop=gq)["alphas"], r["alphas"])


def test_six_step_inputs_force_the_pattern():
    st, props, sse = six_step_case()
    for t in range(6):
        st = accept_np(st, props[t], sse[t], 1.0, 0, CHAIN0, SEED, t & 1)
        a = st["alphas"][:, t + 1]
        assert np.array_equal(a, [np.inf if SIX_PATTERN[c][t] == "A" else 0.0 for c in range(3)])
    assert np.array_equal(st["kcur"][0], [4, 2, 4]) and np.array_equal(st["nacc"], [4, 2, 4])
    assert np.array_equal(st["mult"], [[1, 3, 1], [2, 3, 2], [1, 1, 1]])
    assert (np.abs(st["hist"][0, 1, :5].astype(np.float64)) == 65504.0).sum() == 1 and (bits(st["hist"][:, :, 5:]) == HIST_SENTINEL).all()


@pytest.mark.parametrize("p", LEAP_P)
@pytest.mark.parametrize("variant", LEAP_VARIANTS)
def test_leapfrog_inputs_keep_the_model_exact(p, variant):
    """What makes the float64 model a bit-for-bit reference: every product is exact (so the kernel's fma and the model's
    multiply + add round the same sum once), and with dyadic momenta the sums of the leap call are exact too -- the longdouble
    model gives the same numbers."""
    C = 2
    rs = np.random.RandomState(p % 1000)
    d = leap_case(p, variant, True)
    z = fake_normals(rs, (C, p))
    ks, es, ok = leap_factors(d["sigma"], d["eps"], 0, d["scale"], d["beta"], C)
    mom, q, kin = begin_np(d["q"], d["g"], z, d["sigma"], d["eps"], d["scale"], d["beta"])
    assert ok and products_exact((0.5 * ks, d["g"]), (es, mom))                      # (begin's half kick = half of a full one)
    z2 = np.square(z.astype(LD))
    for c in range(C):
        for k, (lo, hi) in enumerate(part_ranges(p, True)):
            n = hi - lo
            assert abs(LD(kin[c, k]) - z2[c, lo:hi].sum()) <= (n + 2) * LD(2.0) ** -53 * z2[c, lo:hi].sum()
    d = leap_case(p, variant, False)
    for last in (0, 1):
        ks, es, ok = leap_factors(d["sigma"], d["eps"], last, d["scale"], d["beta"], C)
        m, qn, kin = leap_np(d["g"], d["mom"], d["q"], d["sigma"], d["eps"], last, d["scale"], d["beta"])
        ml, ql, kl = leap_np(d["g"], d["mom"], d["q"], d["sigma"], d["eps"], last, d["scale"], d["beta"], ft=LD)
        assert ok and products_exact((ks, d["g"]), (es, m), (m, m))
        assert np.array_equal(m.astype(LD), ml) and np.array_equal(qn.astype(LD), ql)
        if last:
            assert np.array_equal(kin.astype(LD), kl) and same(qn, d["q"])
            assert np.array_equal(kin, np.array([[np.square(m[c, lo:hi])[::-1].sum() for lo, hi in part_ranges(p, False)] for c in range(C)]))
            bad = leap_np(d["g"], d["mom"], d["q"], d["sigma"], d["eps"], 1, d["scale"], d["beta"], mutate="parts_touched")[2]
            chunk = -(-p // hmc_parts(p))                                           # (one workgroup, or chunks of whole trips: nothing to run into)
            assert same(bad, kin) == (hmc_parts(p) == 1 or chunk % 1024 == 0)


def test_part_ranges_tile_the_row():
    for p in LEAP_P + HMC_P + (1024, 2047, 131071):
        for pairs in (False, True):
            r = part_ranges(p, pairs)
            assert len(r) == hmc_parts(p) and r[0][0] == 0 and r[-1][1] == p
            assert all(a[1] == b[0] for a, b in zip(r, r[1:])) and all(lo <= hi for lo, hi in r)
            if pairs:
                assert all(lo % 2 == 0 for lo, hi in r)
    assert hmc_parts(65536) == 64 and hmc_parts(65537) == 64 and hmc_parts(1025) == 2 and hmc_parts(1024) == 1
    assert part_ranges(65537, False)[1] == (1025, 2050) and part_ranges(65537, True)[1] == (1026, 2052)
    assert np.array_equal(parts_touched(65537, 0, wrong=True), np.concatenate([np.arange(1025), [1280, 1536, 1792]]))


def test_fixed_order_sum_is_a_sum():
    rs = np.random.RandomState(0)
    z = fake_normals(rs, (3001,))
    for lo, hi in ((0, 1), (0, 2), (2, 515), (0, 3001), (512, 3000)):
        ref = np.square(z[lo:hi].astype(LD)).sum()
        assert abs(LD(fixed_order_sum_of_squares(z, lo, hi)) - ref) <= (hi - lo + 2) * LD(2.0) ** -53 * ref
    assert fixed_order_sum_of_squares(z, 0, 2) == z[0] ** 2 + z[1] ** 2 and fixed_order_sum_of_squares(z, 4, 4) == 0.0
