"""GPU: the VI, batched-Adam and predictive-moment kernels at the end of csrc/qn_api.hip (k_vi_sample_kl, k_vi_grad, k_adam,
k_pred_moments) through the C ABI, each against a plain numpy reference in np.longdouble written from the header's contract
(include/quinn_amd.h: qn_vi_sample_kl, qn_vi_grad, qn_adam_batched, qn_pred_moments) and the torch formulas the kernels
cite: Normal.log_prob's ordering, the mixture log(pi e^lp1 + (1 - pi) e^lp2), torch.optim.Adam (no amsgrad, L2 weight
decay), np.mean / np.var(ddof=1).  Nothing of quinn_amd enters a reference; only `_lib` is used, to call the library.

The bars hold no fitted constant.  u = 2^-53.
  elementwise result: n_ops * u * (the largest intermediate of that element); n_ops = the rounded operations on the way to
    the result, an exp / log / sqrt call counting 2 (an allowance of 1 ulp = 2 u), counted in comments beside the kernel
    lines (N_* below repeat them).
  reduction of n terms: (n + n_ops) * u * sum|term|, the sum in longdouble.
float32 inputs are rounded ONCE, in the test; the reference converts those float32 values to longdouble.
What an intermediate is, where it is not obvious: a result formed through a cancelling subtraction carries the error of the
operands, so the operands' sizes are intermediates (w = mu + sigma eps: |mu|, |sigma eps|; Adam's g = G gscale + wd W: both
products; the mixture weights r_k = a_k / (a_1 + a_2): their relative error is the ABSOLUTE error of the two log densities,
which enters the result times r_1 r_2 |gp_1 - gp_2|).  For dmu / drho and for Adam's W this reads "largest intermediate" more
generously than a plain maximum: the magnitude is a first-order error bound (`mgp`, `mag_mu`, `mag_rho` in _ref_vi_grad: the
weighted |gp_k| summed plus that weight term; `cond` in _ref_adam: v's relative error through a cancelling g).  Each test prints `ratio <kernel> <dtype> <quantity> <worst err/bar>`;
profiles/elementwise_kernels.txt records them."""
import math

import numpy as np
import pytest
import torch

from quinn_amd import _lib

pytestmark = pytest.mark.gpu

LD = np.longdouble
U = LD(2.0) ** -53
LOG_SQRT_2PI = np.log(np.sqrt(LD(2) * np.arctan(LD(1)) * 4))           # log(sqrt(2 pi)), pi in longdouble
SENT = -7.25                                                            # sentinel after every output; exact in float32
PAD = 16

# rounded operations, as counted beside the kernel lines in csrc/qn_api.hip
N_W = 4                 # exp, mul, add
N_LOGQ = 19
N_LOGP = 23
N_ADAM_M, N_ADAM_V, N_ADAM_W = 6, 10, 18
N_MEAN, N_VAR = 1, 3


def N_VIGRAD(S):
    return 36 + S


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def _out(n, dtype=torch.float64):
    """n outputs followed by PAD sentinels."""
    return torch.full((n + PAD,), SENT, dtype=dtype, device="cuda")


def _take(buf, n):
    """(the n outputs on the host, as float64 if they are) after checking that the sentinels behind them are untouched."""
    h = buf.cpu().numpy()
    assert np.all(h[n:] == SENT), "sentinel after the output overwritten"
    return h[:n].copy()


def _ptr(t):
    return None if t is None else t.data_ptr()


def _ratio(what, err, bar):
    """Worst err / bar over the finite entries (bar == 0 where the result must be exact: then err must be 0)."""
    err, bar = np.atleast_1d(np.asarray(err, dtype=LD)), np.atleast_1d(np.asarray(bar, dtype=LD))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bar > 0, err / np.where(bar > 0, bar, 1), np.where(err == 0, 0, np.inf))
    worst = float(np.max(r)) if r.size else 0.0
    print("ratio %s %.4f" % (what, worst))
    return worst


def _dt(dtype):
    return (_lib.QN_F64, torch.float64, np.float64) if dtype == "float64" else (_lib.QN_F32, torch.float32, np.float32)


# ------------------------------------------------------------------------------------------------ qn_vi_sample_kl
def _lognormal(w, s):
    """torch.distributions.Normal(0, s).log_prob(w): -(w^2) / (2 s^2) - log(s) - log(sqrt(2 pi)), longdouble."""
    s = LD(s)
    return -(w * w) / (2 * s * s) - np.log(s) - LOG_SQRT_2PI


def _ref_sample_kl(mu, rho, eps, pi, s1, s2):
    """-> W [S, p], logq [S], logp [S], sum|term| of both, the largest intermediate of every W (all longdouble)."""
    mu, rho, eps, pi = mu.astype(LD), rho.astype(LD), eps.astype(LD), LD(pi)
    sig = np.exp(rho)
    w = mu + sig * eps
    quad = (w - mu) ** 2 / (2 * sig * sig)
    logq = (-LOG_SQRT_2PI - rho - quad).sum(axis=1)
    absq = np.abs(-LOG_SQRT_2PI - rho - quad).sum(axis=1)
    with np.errstate(divide="ignore", under="ignore"):
        term = np.log(pi * np.exp(_lognormal(w, s1)) + (1 - pi) * np.exp(_lognormal(w, s2)))
    wmag = np.maximum(np.maximum(np.abs(mu)[None, :], np.abs(sig * eps)), np.abs(w))
    return w, logq, term.sum(axis=1), absq, np.abs(term).sum(axis=1), wmag


def _run_sample_kl(mu, rho, eps, pi, s1, s2, dtype):
    S, p = eps.shape
    code, tdt, _ = _dt(dtype)
    W, lq, lp = _out(S * p, tdt), _out(S), _out(S)
    mu, rho, eps = _dev(mu), _dev(rho), _dev(eps)                          # (named: the inputs live until the kernel has run)
    _lib.check(_lib.lib().qn_vi_sample_kl(mu.data_ptr(), rho.data_ptr(), eps.data_ptr(), S, p, pi, s1, s2, code,
                                          W.data_ptr(), lq.data_ptr(), lp.data_ptr(), None), "qn_vi_sample_kl")
    torch.cuda.synchronize()
    return _take(W, S * p).reshape(S, p), _take(lq, S), _take(lp, S)


def _vi_inputs(S, p, seed):
    rs = np.random.RandomState(seed)
    mu = 0.3 * rs.randn(p)
    rho = rs.uniform(-1.5, 0.0, p)
    eps = rs.randn(S, p)                                                  # a row of its own per sample: a wrong s * p offset shows
    return mu, rho, eps


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("p", [1, 63, 64, 65, 1023, 1024, 1025, 2049])
@pytest.mark.parametrize("S", [1, 3])
def test_vi_sample_kl_matches_the_longdouble_reference(S, p, dtype):
    """W_out, logq, logp of every sample.  The prior (0.25, 1.5, 0.5) has log densities whose three summands share a sign, so
    that |term| is as large as its intermediates (the reduction bar is stated in sum|term|).
    float64 W_out: within the elementwise bar of the longdouble value.  Against numpy's float64 mu + exp(rho) * eps it is NOT bit
    for bit (observed on gfx950: between two thirds and all of a case's entries are equal, the rest differ by at most 2.25 ulp of
    the element's largest intermediate, which is many ulps of w where mu and sigma * eps cancel): the compiler contracts
    mu + sigma * eps into one fma and the device exp differs from numpy's in the last place for some arguments.  So numpy's
    value is printed beside the bar, not asserted (profiles/elementwise_kernels.txt).
    float32 W_out: float32(the float64 W_out of the same inputs), bit for bit."""
    mu, rho, eps = _vi_inputs(S, p, 1000 * S + p)
    pi, s1, s2 = 0.25, 1.5, 0.5
    w, logq, logp, absq, absp, wmag = _ref_sample_kl(mu, rho, eps, pi, s1, s2)
    W64, lq, lp = _run_sample_kl(mu, rho, eps, pi, s1, s2, "float64")
    tag = "vi_sample_kl %s S=%d p=%d" % (dtype, S, p)
    if dtype == "float32":
        W32, lq32, lp32 = _run_sample_kl(mu, rho, eps, pi, s1, s2, "float32")
        assert W32.dtype == np.float32 and np.array_equal(W32, W64.astype(np.float32))
        assert np.array_equal(lq32, lq) and np.array_equal(lp32, lp)          # the sums do not depend on the output type
    r = [_ratio(tag + " W", np.abs(W64.astype(LD) - w), N_W * U * wmag),
         _ratio(tag + " logq", np.abs(lq.astype(LD) - logq), (p + N_LOGQ) * U * absq),
         _ratio(tag + " logp", np.abs(lp.astype(LD) - logp), (p + N_LOGP) * U * absp)]
    wnp = mu + np.exp(rho) * eps
    ulps = np.abs(W64 - wnp) / np.spacing(wmag.astype(np.float64))
    print("ulps %s W-vs-numpy max %.2f bit-equal %.4f" % (tag, ulps.max(), np.mean(W64 == wnp)))
    assert max(r) <= 1.0, r


# ------------------------------------------------------------------------------------------------ qn_vi_grad
def _ref_vi_grad(mu, rho, eps, gW, pi, s1, s2, gw_scale, kl_scale):
    """-> dmu, drho [p] and the largest-intermediate magnitude of each (longdouble)."""
    mu, rho, eps, g = mu.astype(LD), rho.astype(LD), eps.astype(LD), gW.astype(LD) * LD(gw_scale)
    pi, s1, s2, kl = LD(pi), LD(s1), LD(s2), LD(kl_scale)
    S = eps.shape[0]
    sig = np.exp(rho)
    se = sig * eps
    w = mu + se
    with np.errstate(divide="ignore", invalid="ignore", under="ignore"):
        a1, a2 = pi * np.exp(_lognormal(w, s1)), (1 - pi) * np.exp(_lognormal(w, s2))
        r1, r2 = a1 / (a1 + a2), a2 / (a1 + a2)
        gp = r1 * (-w / (s1 * s1)) + r2 * (-w / (s2 * s2))
    dmu = g.sum(axis=0) - kl * (gp.sum(axis=0) / S)
    drho = (g * se).sum(axis=0) - kl * (1 + (gp * se).sum(axis=0) / S)
    # magnitudes: |w|'s operands; the log densities' largest summand (its absolute error is the weights' relative error)
    wm = np.maximum(np.maximum(np.abs(mu)[None, :], np.abs(se)), np.abs(w))
    L = sum(np.maximum(np.maximum(w * w / (2 * s * s), abs(np.log(s))), LOG_SQRT_2PI) for s in (s1, s2))
    mgp = r1 * wm / (s1 * s1) + r2 * wm / (s2 * s2) + r1 * r2 * wm * abs(1 / (s1 * s1) - 1 / (s2 * s2)) * L
    mag_mu = np.abs(g).sum(axis=0) + kl * mgp.sum(axis=0) / S
    mag_rho = np.abs(g * se).sum(axis=0) + kl * (1 + (mgp * np.abs(se)).sum(axis=0) / S)
    return dmu, drho, mag_mu, mag_rho


def _run_vi_grad(mu, rho, eps, gW, pi, s1, s2, gw_scale, kl_scale, dtype):
    S, p = eps.shape
    code = _dt(dtype)[0]
    dmu, drho = _out(p), _out(p)
    mu, rho, eps, gW = _dev(mu), _dev(rho), _dev(eps), _dev(gW)
    _lib.check(_lib.lib().qn_vi_grad(mu.data_ptr(), rho.data_ptr(), eps.data_ptr(), gW.data_ptr(), S, p, pi,
                                     s1, s2, gw_scale, kl_scale, code, dmu.data_ptr(), drho.data_ptr(), None), "qn_vi_grad")
    torch.cuda.synchronize()
    return _take(dmu, p), _take(drho, p)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("prior", [(0.5, 1.0, 1.0), (0.25, 0.5, 0.1), (1.0, 2.0, 0.0025)])
@pytest.mark.parametrize("p", [1, 255, 256, 257, 700])
@pytest.mark.parametrize("S", [1, 2, 5])
def test_vi_grad_matches_the_longdouble_chain_rule(S, p, prior, dtype):
    mu, rho, eps = _vi_inputs(S, p, 7000 + 10 * S + p)
    rs = np.random.RandomState(S * p + 1)
    gW = (40.0 * rs.randn(S, p)).astype(_dt(dtype)[2])                      # float32: rounded once, here
    gw_scale, kl_scale = 0.0371, 0.013                                       # both != 1
    dmu, drho, mag_mu, mag_rho = _ref_vi_grad(mu, rho, eps, gW, *prior, gw_scale, kl_scale)
    k_mu, k_rho = _run_vi_grad(mu, rho, eps, gW, *prior, gw_scale, kl_scale, dtype)
    tag = "vi_grad %s S=%d p=%d prior=%s" % (dtype, S, p, prior)
    r = [_ratio(tag + " dmu", np.abs(k_mu.astype(LD) - dmu), N_VIGRAD(S) * U * mag_mu),
         _ratio(tag + " drho", np.abs(k_rho.astype(LD) - drho), N_VIGRAD(S) * U * mag_rho)]
    assert max(r) <= 1.0, r


# ------------------------------------------------------------------------------------------------ underflow semantics
def _underflow_inputs():
    """S = 3, prior (0.5, 0.01, 0.0025).  Three groups of elements, 40 each (p = 120):
      A  |w| <= 0.04 in every sample: neither component underflows (exponents >= -128);
      B  0.15 <= |w| <= 0.3 in every sample: exp of the sigma2 component's log density (<= -1800) is 0, sigma1's is not (>= -450);
      C  as A in samples 0 and 2, |w| ~ 1 in sample 1: there both are 0 (exponents -5000 and -80000): log(0), 0/0.
    No exponent lies near the underflow threshold (-708 .. -745), where a last-place difference of exp would decide."""
    rs = np.random.RandomState(5)
    n, S = 40, 3
    sgn = np.where(rs.rand(3 * n) < 0.5, -1.0, 1.0)
    mu = np.concatenate([rs.uniform(0.005, 0.03, n), rs.uniform(0.17, 0.28, n), rs.uniform(0.005, 0.03, n)]) * sgn
    rho = np.log(np.concatenate([np.full(n, 0.004), np.full(n, 0.008), np.full(n, 0.5)]))
    eps = rs.uniform(-2.0, 2.0, (S, 3 * n))
    eps[:, 2 * n:] = rs.uniform(-0.01, 0.01, (S, n))
    eps[1, 2 * n:] = 2.0 * sgn[2 * n:]
    kind = np.repeat(np.array(["A", "B", "C"]), n)
    return mu, rho, eps, kind, (0.5, 0.01, 0.0025)


def _torch_vi(mu, rho, eps, gW, pi, s1, s2, gw_scale, kl_scale):
    """The reference's own formulation in torch float64 on the CPU: W = mu + exp(rho) eps, Normal.log_prob, the mixture through
    exp and log, viloss = (mean logq - mean logp) kl_scale + <gW gw_scale, W>, autograd to (mu, rho)."""
    N = torch.distributions.Normal
    tmu, trho = torch.tensor(mu, requires_grad=True), torch.tensor(rho, requires_grad=True)
    teps = torch.tensor(eps)
    sig = torch.exp(trho)
    W = tmu + sig * teps
    logq = N(tmu, sig).log_prob(W).sum(dim=1)
    logp = torch.log(pi * torch.exp(N(0.0, s1).log_prob(W)) + (1.0 - pi) * torch.exp(N(0.0, s2).log_prob(W))).sum(dim=1)
    loss = (logq.mean() - logp.mean()) * kl_scale + (torch.tensor(gW, dtype=torch.float64) * gw_scale * W).sum()
    loss.backward()
    return logp.detach().numpy(), tmu.grad.numpy(), trho.grad.numpy()


def _same_pattern(a, b):
    return (np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.isposinf(a), np.isposinf(b))
            and np.array_equal(np.isneginf(a), np.isneginf(b)))


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_underflowing_mixture_components_give_torchs_inf_nan_pattern(dtype):
    """-inf in logp and NaN in dmu / drho exactly where torch has them; every finite entry within its bar."""
    mu, rho, eps, kind, prior = _underflow_inputs()
    S, p = eps.shape
    gW = (3.0 * np.random.RandomState(6).randn(S, p)).astype(_dt(dtype)[2])
    gw_scale, kl_scale = 0.25, 0.5
    t_logp, t_dmu, t_drho = _torch_vi(mu, rho, eps, gW, *prior, gw_scale, kl_scale)
    # the inputs do what their description says
    assert np.isneginf(t_logp).tolist() == [False, True, False]
    assert np.all(np.isnan(t_dmu) == (kind == "C")) and np.all(np.isnan(t_drho) == (kind == "C"))
    w, logq, logp, absq, absp, wmag = _ref_sample_kl(mu, rho, eps, *prior)
    p2 = np.exp(-(w * w) / LD(2 * 0.0025 ** 2)).astype(np.float64)
    assert np.all(p2[:, kind == "B"] == 0) and np.all(p2[:, kind == "A"] > 0)

    W, lq, lp = _run_sample_kl(mu, rho, eps, *prior, dtype)
    assert _same_pattern(lp, t_logp) and np.all(np.isfinite(lq)) and np.all(np.isfinite(W))
    fin = np.isfinite(lp)
    k_mu, k_rho = _run_vi_grad(mu, rho, eps, gW, *prior, gw_scale, kl_scale, dtype)
    assert _same_pattern(k_mu, t_dmu) and _same_pattern(k_rho, t_drho)
    dmu, drho, mag_mu, mag_rho = _ref_vi_grad(mu, rho, eps, gW, *prior, gw_scale, kl_scale)
    ok = kind != "C"
    tag = "vi_underflow %s" % dtype
    r = [_ratio(tag + " logq", np.abs(lq.astype(LD) - logq), (p + N_LOGQ) * U * absq),
         _ratio(tag + " logp", np.abs(lp[fin].astype(LD) - logp[fin]), (p + N_LOGP) * U * absp[fin]),
         _ratio(tag + " dmu", np.abs(k_mu[ok].astype(LD) - dmu[ok]), N_VIGRAD(S) * U * mag_mu[ok]),
         _ratio(tag + " drho", np.abs(k_rho[ok].astype(LD) - drho[ok]), N_VIGRAD(S) * U * mag_rho[ok])]
    assert max(r) <= 1.0, r


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_a_component_of_weight_zero_changes_nothing(dtype):
    """pi = 1.0 with sigma2 = 0.0025 and |w| of a few tenths: the second component is 0 * exp(-huge) = 0 * 0; everything stays
    finite, equals torch's pattern, and equals the one-component values."""
    mu, rho, eps = _vi_inputs(2, 300, 77)
    prior = (1.0, 2.0, 0.0025)
    gW = np.random.RandomState(8).randn(2, 300).astype(_dt(dtype)[2])
    t_logp, t_dmu, t_drho = _torch_vi(mu, rho, eps, gW, *prior, 0.5, 2.0)
    W, lq, lp = _run_sample_kl(mu, rho, eps, *prior, dtype)
    k_mu, k_rho = _run_vi_grad(mu, rho, eps, gW, *prior, 0.5, 2.0, dtype)
    assert np.all(np.isfinite(t_logp)) and np.all(np.isfinite(t_dmu)) and np.all(np.isfinite(t_drho))
    assert _same_pattern(lp, t_logp) and _same_pattern(k_mu, t_dmu) and _same_pattern(k_rho, t_drho)
    w, logq, logp, absq, absp, wmag = _ref_sample_kl(mu, rho, eps, *prior)
    dmu, drho, mag_mu, mag_rho = _ref_vi_grad(mu, rho, eps, gW, *prior, 0.5, 2.0)
    tag = "vi_pi_one %s" % dtype
    r = [_ratio(tag + " logp", np.abs(lp.astype(LD) - logp), (300 + N_LOGP) * U * absp),
         _ratio(tag + " dmu", np.abs(k_mu.astype(LD) - dmu), N_VIGRAD(2) * U * mag_mu),
         _ratio(tag + " drho", np.abs(k_rho.astype(LD) - drho), N_VIGRAD(2) * U * mag_rho)]
    assert max(r) <= 1.0, r


# ------------------------------------------------------------------------------------------------ qn_adam_batched
B1, B2, AEPS = 0.9, 0.999, 1e-8


def _adam_scalars(lr, step):
    """torch.optim.Adam forms its bias corrections and step size as Python floats (float64): so does the reference."""
    bc1 = 1 - B1 ** step
    bc2s = math.sqrt(1 - B2 ** step)
    return [l / bc1 for l in lr], bc2s


def _ref_adam(W, G, m, v, lr, gscale, wd, step):
    """One torch.optim.Adam step (single-tensor order, no amsgrad, L2 weight decay) for every member with lr != 0, in
    longdouble -> W, m, v and the largest-intermediate magnitude of each."""
    W, G, m, v = W.astype(LD), G.astype(LD), m.astype(LD), v.astype(LD)
    step_size, bc2s = _adam_scalars(lr, step)
    ss = np.array(step_size, dtype=LD)[:, None]
    b1, b2 = LD(B1), LD(B2)
    g = G * LD(gscale) + LD(wd) * W
    gmag = np.maximum(np.abs(G * LD(gscale)), np.abs(LD(wd) * W))
    mm = m + (1 - b1) * (g - m)
    vv = v * b2 + (1 - b2) * g * g
    denom = np.sqrt(vv) / LD(bc2s) + LD(AEPS)
    Wn = W - ss * (mm / denom)
    mag_m = np.maximum(np.maximum(gmag, np.abs(m)), np.abs(mm))
    mag_v = np.maximum(v * b2 + (1 - b2) * gmag * gmag, vv)
    with np.errstate(divide="ignore", invalid="ignore"):
        cond = np.where(vv > 0, mag_v / np.where(vv > 0, vv, 1), 1)           # g^2 through a cancelling g: v's relative error
    mag_w = np.maximum(np.abs(W), np.maximum(np.abs(Wn), ss * (mag_m / denom) * cond))
    return Wn, mm, vv, mag_w, mag_m, mag_v


def _run_adam(W, G, m, v, lr, gscale, wd, step, dtype):
    B, p = W.shape
    code = _dt(dtype)[0]
    bufs = []
    for a in (W, m, v):
        t = _out(B * p)
        t[:B * p] = _dev(a).reshape(-1)
        bufs.append(t)
    G, lr = _dev(G), _dev(np.asarray(lr, dtype=np.float64))
    _lib.check(_lib.lib().qn_adam_batched(bufs[0].data_ptr(), G.data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(),
                                          lr.data_ptr(), B, p, code, gscale, wd, B1, B2, AEPS,
                                          step, None), "qn_adam_batched")
    torch.cuda.synchronize()
    return [_take(t, B * p).reshape(B, p) for t in bufs]


def _adam_inputs(B, p, dtype, seed):
    rs = np.random.RandomState(seed)
    W = rs.randn(B, p)
    G = (5.0 * rs.randn(B, p)).astype(_dt(dtype)[2])                          # float32: rounded once, here
    m = 0.5 * rs.randn(B, p)
    v = rs.uniform(0.01, 4.0, (B, p))
    return W, G, m, v


P_STRIDE = 1024 * 256 + 3        # past the 1024 x 256 threads of the capped grid: the second grid-stride pass does the tail


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("step", [1, 2, 1000])
@pytest.mark.parametrize("wd", [0.0, 0.1])
@pytest.mark.parametrize("p", [1, 255, 257, P_STRIDE])
@pytest.mark.parametrize("B", [1, 3])
def test_adam_step_matches_the_longdouble_reference_and_freezes_lr_zero(B, p, wd, step, dtype):
    """Live members against the longdouble step; with B = 3 the middle member has lr == 0 (the header: "Members with lr[b] == 0
    are left untouched", which is what the kernel's early return does): its W, m, v are the inputs bit for bit."""
    W, G, m, v = _adam_inputs(B, p, dtype, 31 * B + p % 1000 + step)
    lr = [3e-3] if B == 1 else [3e-3, 0.0, 0.02]
    gscale = 0.37
    Wn, mn, vn, mag_w, mag_m, mag_v = _ref_adam(W, G, m, v, lr, gscale, wd, step)
    kW, km, kv = _run_adam(W, G, m, v, lr, gscale, wd, step, dtype)
    live = [b for b in range(B) if lr[b] != 0.0]
    for b in range(B):
        if lr[b] == 0.0:
            assert np.array_equal(kW[b], W[b]) and np.array_equal(km[b], m[b]) and np.array_equal(kv[b], v[b])
    tag = "adam %s B=%d p=%d wd=%g step=%d" % (dtype, B, p, wd, step)
    r = [_ratio(tag + " W", np.abs(kW[live].astype(LD) - Wn[live]), N_ADAM_W * U * mag_w[live]),
         _ratio(tag + " m", np.abs(km[live].astype(LD) - mn[live]), N_ADAM_M * U * mag_m[live]),
         _ratio(tag + " v", np.abs(kv[live].astype(LD) - vn[live]), N_ADAM_V * U * mag_v[live])]
    assert max(r) <= 1.0, r


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("step", [1, 5])
def test_adam_zero_gradient_on_zero_state_is_a_step_of_exactly_zero(step, dtype):
    """G = 0, m = v = 0, no weight decay: 0 / (sqrt(0) / c + eps) = 0, W unchanged bit for bit, m and v stay 0, no NaN.  Every
    second element has a gradient, so that the kernel demonstrably ran."""
    rs = np.random.RandomState(3)
    B, p = 2, 300
    W = rs.randn(B, p)
    G = rs.randn(B, p).astype(_dt(dtype)[2])
    G[:, ::2] = 0.0
    z = np.zeros((B, p))
    kW, km, kv = _run_adam(W, G, z, z, [1e-2, 0.5], 1.0, 0.0, step, dtype)
    assert np.all(np.isfinite(kW)) and np.all(np.isfinite(km)) and np.all(np.isfinite(kv))
    assert np.array_equal(kW[:, ::2], W[:, ::2]) and np.all(km[:, ::2] == 0.0) and np.all(kv[:, ::2] == 0.0)
    assert np.all(kW[:, 1::2] != W[:, 1::2])


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("wd", [0.0, 0.1])
def test_adam_steps_match_torch_optim_adam_on_the_cpu(wd, dtype):
    """Steps 1, 2, 3 from m = v = 0, carrying the kernel's own m and v, against torch.optim.Adam (CPU, float64, one optimiser
    per member since the learning rates differ) on the same weights and gradients.  Bar: the elementwise bar of one step
    (n_ops * u * largest intermediate, as against the longdouble reference), at every step, although both sides round and the
    state is carried."""
    rs = np.random.RandomState(11)
    B, p = 2, 257
    lr, gscale = [3e-3, 0.02], 0.37
    W0 = rs.randn(B, p)
    Gs = [(5.0 * rs.randn(B, p)).astype(_dt(dtype)[2]) for _ in range(3)]
    params = [torch.tensor(W0[b].copy(), requires_grad=True) for b in range(B)]
    opts = [torch.optim.Adam([params[b]], lr=lr[b], betas=(B1, B2), eps=AEPS, weight_decay=wd, amsgrad=False, foreach=False)
            for b in range(B)]
    W, m, v = W0, np.zeros((B, p)), np.zeros((B, p))
    for step in (1, 2, 3):
        G = Gs[step - 1]
        for b in range(B):
            params[b].grad = torch.tensor(G[b].astype(np.float64) * gscale)
            opts[b].step()
        ref = _ref_adam(W, G, m, v, lr, gscale, wd, step)
        W, m, v = _run_adam(W, G, m, v, lr, gscale, wd, step, dtype)
        bars = [N_ADAM_W * U * ref[3], N_ADAM_M * U * ref[4], N_ADAM_V * U * ref[5]]
        tW = np.stack([params[b].detach().numpy() for b in range(B)])
        tm = np.stack([opts[b].state[params[b]]["exp_avg"].numpy() for b in range(B)])
        tv = np.stack([opts[b].state[params[b]]["exp_avg_sq"].numpy() for b in range(B)])
        tag = "adam_vs_torch %s wd=%g step=%d" % (dtype, wd, step)
        r = [_ratio(tag + " W", np.abs(W.astype(LD) - tW.astype(LD)), bars[0]),
             _ratio(tag + " m", np.abs(m.astype(LD) - tm.astype(LD)), bars[1]),
             _ratio(tag + " v", np.abs(v.astype(LD) - tv.astype(LD)), bars[2])]
        assert max(r) <= 1.0, (step, r)


# ------------------------------------------------------------------------------------------------ qn_pred_moments
def _moment_inputs(M, K, dtype):
    """Random members; from K >= 3 on, column 1 has all members equal (-2.75: M * y and the mean are exact, the variance must
    be exactly 0) and column 2 has mean 1e8 and spread 1e-3.  Column 2's offsets are multiples of 2^-10 that sum to 0: the
    partial sums and the float64 mean are then exact.  (A float64 mean off by d leaves M d^2 in the sum of squares of ANY
    two-pass form, np.var included; that is outside a bar stated in sum|term| and is not what the column is for.  A one-pass
    sum(y^2) - sum(y)^2 / M form would be off by ~1e16 * 2^-53 against a variance of 1e-6.)  As float32 the column is 1e8 in
    every member: the reference sees those values."""
    rs = np.random.RandomState(100 * M + K)
    Y = rs.randn(M, K) + 0.5
    if K >= 3:
        Y[:, 1] = -2.75
        k = rs.randint(-3, 4, M).astype(np.float64)
        k[-1] -= k.sum()                                                   # the offsets sum to 0
        if M == 1:
            k[:] = 0
        Y[:, 2] = 1e8 + k * 2.0 ** -10
    return Y.astype(_dt(dtype)[2])


def _run_moments(Y, dtype, want_var):
    M, K = Y.shape
    mean, var = _out(K), (_out(K) if want_var else None)
    Yd = _dev(Y)
    _lib.check(_lib.lib().qn_pred_moments(Yd.data_ptr(), _dt(dtype)[0], M, K, mean.data_ptr(), _ptr(var), None),
               "qn_pred_moments")
    torch.cuda.synchronize()
    return _take(mean, K), (_take(var, K) if want_var else None)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("M,K,want_var", [(1, 5, False)] + [(M, K, wv) for M, K in [(2, 1), (2, 257), (7, 256), (33, 1000)]
                                                            for wv in (False, True)])
def test_pred_moments_match_longdouble_mean_and_unbiased_variance(M, K, want_var, dtype):
    """np.mean / np.var(ddof=1) over the members in longdouble; a null var_out skips the variance (the only form M == 1 takes:
    the non-null call is an argument error, tests/test_host_api_errors.py)."""
    Y = _moment_inputs(M, K, dtype)
    Yl = Y.astype(LD)
    mean = np.mean(Yl, axis=0)
    k_mean, k_var = _run_moments(Y, dtype, want_var)
    tag = "pred_moments %s M=%d K=%d var=%d" % (dtype, M, K, want_var)
    r = [_ratio(tag + " mean", np.abs(k_mean.astype(LD) - mean), (M + N_MEAN) * U * np.abs(Yl).sum(axis=0) / M)]
    if want_var:
        var = np.var(Yl, axis=0, ddof=1)
        terms = ((Yl - mean) ** 2).sum(axis=0) / (M - 1)
        r.append(_ratio(tag + " var", np.abs(k_var.astype(LD) - var), (M + N_VAR) * U * terms))
        assert np.all(k_var >= 0.0)
        if K >= 3:
            assert k_var[1] == 0.0 and k_mean[1] == -2.75
            assert k_mean[2] == 1e8
            if dtype == "float64":
                assert k_var[2] > 0.0 or np.all(Y[:, 2] == 1e8)
            else:
                assert k_var[2] == 0.0
    assert max(r) <= 1.0, r
