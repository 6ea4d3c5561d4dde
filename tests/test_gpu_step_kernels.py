"""GPU: the accept kernel (`k_accept`, csrc/qn_mcmc.hip) and the leapfrog kernels (`k_hmc_begin` / `k_hmc_leap`,
csrc/qn_hmc_leap.hip) called directly through the C ABI and held to the host model of tests/test_step_ref_cpu.py.

Everything is compared bit for bit except `alphas` = exp(..), which is held to 4 ulp of numpy's longdouble exp (OCML documents
1 ulp for the double exp; the rest is the rounding of the argument and of the reference), and one leapfrog case with inputs
that are not dyadic, held to the elementwise bar of tests/test_gpu_elementwise_kernels.py.  The inputs, and why the model is
exact on them, are in that file; its checks without a device show that these inputs tell the wrong variants from the right one.

Every array a kernel may write is followed by 64 guard bytes that must survive, rows and slots that must not be written are NaN /
sentinel-filled, and whole arrays are compared, so a second writer shows.  `-s` prints the figures of profiles/step_kernels.txt."""
import numpy as np
import pytest

from test_step_ref_cpu import (CHAIN0, HMC_BETA, HMC_P, HMC_TARGET, LD, LEAP_P, LEAP_VARIANTS, NPARTS, SEED, SEED2, SIX_PATTERN, SPECIAL,
                               accept_np, begin_np, bits, dyadic, hmc_case, hmc_parts, leap_case, leap_factors, leap_np,
                               lsum, new_state, part_ranges, parts_case, products_exact, same, six_step_case, special_case,
                               threshold_sse, threshold_state, tie_candidates, ulps)

pytestmark = pytest.mark.gpu

GUARD = 64
ULP_BAR = 4.0


def _L():
    from quinn_amd import _lib
    return _lib, _lib.lib()


class Dev:
    """named device buffers, each followed by GUARD bytes of 0xA5 that get() requires to be intact"""

    def __init__(self, **arrays):
        self.t, self.meta = {}, {}
        for k, v in arrays.items():
            self.put(k, v)

    def put(self, name, a):
        import torch
        if a is None:
            self.t[name] = None
            return
        a = np.ascontiguousarray(a)
        raw = np.concatenate([a.reshape(-1).view(np.uint8), np.full(GUARD, 0xA5, dtype=np.uint8)])
        self.t[name], self.meta[name] = torch.from_numpy(raw).cuda(), (a.shape, a.dtype)

    def ptr(self, name, offset=0):
        t = self.t.get(name)
        return None if t is None else t.data_ptr() + offset

    def get(self, name):
        raw = self.t[name].cpu().numpy()
        shape, dtype = self.meta[name]
        assert (raw[-GUARD:] == 0xA5).all(), f"{name}: written past its end"
        return raw[:-GUARD].view(dtype).reshape(shape)


STATE = ("cur", "cur_lp", "best", "best_lp", "chain", "lps", "alphas", "nacc", "step_ptr", "grad_cur", "x0", "hist", "hscale", "mult",
         "kcur", "sumx")


def _upload(st, **more):
    return Dev(**{k: st.get(k) for k in STATE}, **more)


def _sync():
    import torch
    torch.cuda.synchronize()


def _mcmc_accept(D, sigma, C, chain0, p, nmcmc, seed, par, nparts=1, kcap=0, pstride=0, nxt=None):
    _lib, L = _L()
    a = (D.ptr("prop"), D.ptr("sse"), sigma, 0, C, chain0, p, nmcmc, seed, D.ptr("cur"), D.ptr("cur_lp"), D.ptr("best"), D.ptr("best_lp"),
         D.ptr("chain"), D.ptr("lps"), D.ptr("alphas"), D.ptr("nacc"), D.ptr("x0"), D.ptr("hist"), D.ptr("hscale"), D.ptr("mult"),
         D.ptr("kcur"), D.ptr("sumx"), kcap, pstride, D.ptr("step_ptr"))
    if nxt is None:
        _lib.check(L.qn_mcmc_accept(*a, par, nparts, None), "qn_mcmc_accept")
    else:
        mode, c1, t_next, s_iso = nxt
        _lib.check(L.qn_mcmc_accept_propose(*a, mode, D.ptr("sd"), c1, D.ptr("delta"), t_next, s_iso, D.ptr("prop_next"), par, nparts, None),
                   "qn_mcmc_accept_propose")
    _sync()


def _hmc_accept(D, sigma, C, chain0, p, nmcmc, seed, par, tempered):
    _lib, L = _L()
    a = (D.ptr("prop"), D.ptr("gprop"), D.ptr("sse"), D.ptr("kin_cur"), D.ptr("kin_prop"), sigma, 0, C, chain0, p, nmcmc, seed, D.ptr("cur"),
         D.ptr("grad_cur"), D.ptr("cur_lp"), D.ptr("best"), D.ptr("best_lp"), D.ptr("chain"), D.ptr("lps"), D.ptr("alphas"), D.ptr("nacc"),
         D.ptr("step_ptr"), par)
    if tempered:
        _lib.check(L.qn_hmc_accept_t(*a, D.ptr("beta"), None), "qn_hmc_accept_t")
    else:
        _lib.check(L.qn_hmc_accept(*a, None), "qn_hmc_accept")
    _sync()


WORST = {"ulp": 0.0}


def _check_state(D, want, what, alpha_ref=None):
    """the whole device state against the model's, bit for bit; alphas against alpha_ref (longdouble, NaN where the model's value
    is exact: 0, inf, NaN or never written) to ULP_BAR"""
    for k in STATE:
        if want.get(k) is None:
            continue
        got = D.get(k)
        if k == "alphas" and alpha_ref is not None:
            live = ~np.isnan(alpha_ref)
            assert same(got[~live], want[k][~live]), (what, k)
            d = ulps(got[live], alpha_ref[live])
            WORST["ulp"] = max(WORST["ulp"], float(d.max()))
            print(f"\nstep_kernels alphas {what}: max ulp distance {float(d.max()):.3f} (bar {ULP_BAR}); worst so far {WORST['ulp']:.3f}")
            assert (d <= ULP_BAR).all(), (what, d)
        else:
            assert same(got, want[k]), (what, k, got, want[k])


def _alpha_ref(st, step, arg):
    ref = np.full(st["alphas"].shape, np.nan, dtype=LD)
    ref[:, step + 1] = np.exp(np.asarray(arg, dtype=LD))
    return ref


# ------------------------------------------------------------------------------------------- A. the decision at the threshold
def _threshold_run(entry, seed, step, par, chain0, C, first=0):
    """a launch of C chains from `chain0` on their threshold inputs (even first + b accept) -> device buffers, model state, .."""
    sse, u, acc = threshold_sse(seed, chain0, C, step, first)
    st = threshold_state(C, 3, step, par, with_grad=entry == "hmc")
    rs = np.random.RandomState(step)
    prop, gprop = dyadic(rs, (C, 3)), dyadic(rs, (C, 3))
    if entry == "hmc":
        zero = np.zeros((C, 1))
        D = _upload(st, prop=prop, sse=sse, gprop=gprop, kin_cur=zero, kin_prop=zero)
        _hmc_accept(D, 1.0, C, chain0, 3, 4, seed, par, False)
        want = accept_np(st, prop, sse, 1.0, 0, chain0, seed, par, kin_cur=zero, kin_prop=zero, gprop=gprop)
    else:
        D = _upload(st, prop=prop, sse=sse)
        _mcmc_accept(D, 1.0, C, chain0, 3, 4, seed, par)
        want = accept_np(st, prop, sse, 1.0, 0, chain0, seed, par)
    return D, st, want, sse, acc


@pytest.mark.parametrize("par", [0, 1])
@pytest.mark.parametrize("step", [0, 3])
@pytest.mark.parametrize("seed", [SEED, SEED2])
@pytest.mark.parametrize("entry", ["mcmc", "hmc"])
def test_decision_at_the_threshold(entry, seed, step, par):
    """mh = u (1 + 2^-40) on even chains, u (1 - 2^-40) on odd ones: even chains accept, odd ones reject -- with the uniform of
    stream 2 step + 1, purpose 2, global chain 5 + b, words 0 and 1, and no other."""
    D, st, want, sse, acc = _threshold_run(entry, seed, step, par, CHAIN0, 8)
    assert np.array_equal(D.get("nacc"), acc.astype(np.int64)) and acc.tolist() == [True, False] * 4
    _check_state(D, want, f"threshold {entry} seed={seed} step={step} par={par}", _alpha_ref(st, step, -0.5 * sse[:, 0]))


@pytest.mark.parametrize("entry", ["mcmc", "hmc"])
def test_decision_uses_the_global_chain_id(entry):
    """chains 5..7 of a launch of 8 from chain 0 == a launch of 3 from chain 5, and chains 0..2 == a launch of 3 from chain 0,
    each on its own threshold inputs"""
    step, par = 3, 1
    D8, st8, want8, sse8, acc8 = _threshold_run(entry, SEED, step, par, 0, 8)
    _check_state(D8, want8, f"global id {entry} 8 chains", _alpha_ref(st8, step, -0.5 * sse8[:, 0]))
    for chain0 in (5, 0):
        D3, st3, want3, sse3, acc3 = _threshold_run(entry, SEED, step, par, chain0, 3, first=chain0)
        assert same(sse3, sse8[chain0:chain0 + 3]) and np.array_equal(acc3, acc8[chain0:chain0 + 3])
        for k in ("alphas", "lps", "nacc"):
            assert same(D3.get(k), D8.get(k)[chain0:chain0 + 3]), (chain0, k)
        _check_state(D3, want3, f"global id {entry} 3 chains from {chain0}", _alpha_ref(st3, step, -0.5 * sse3[:, 0]))


def test_a_tie_rejects():
    """u < mh is strict.  65 single-chain launches of the same global chain and step (the same u) with mh stepping through the
    doubles around u: each decision must be u < mh for the mh THE DEVICE reports in alphas, and one of them is mh == u exactly
    (x = log u has a finer grid than u in (0.61, 0.77): consecutive x move exp(x) by 0.3 .. 0.4 of u's last place)."""
    c, u, sse = tie_candidates(SEED, range(64), 1, 32)
    mhs = []
    for i in range(sse.size):
        st = threshold_state(1, 3, 1, 1)
        D = _upload(st, prop=st["cur"] + 1.0, sse=sse[i:i + 1].reshape(1, 1))
        _mcmc_accept(D, 1.0, 1, c, 3, 4, SEED, 1)
        mh = D.get("alphas")[0, 2]
        mhs.append(mh)
        assert D.get("nacc")[0] == int(u < mh), (i, u, mh)
        assert same(D.get("cur")[0], st["cur"][0] + 1.0 if u < mh else st["cur"][0])
    mhs = np.array(mhs)
    assert mhs[0] > u > mhs[-1]
    print(f"\nstep_kernels tie: {int((mhs == u).sum())} of {mhs.size} launches had mh == u exactly")
    assert (mhs == u).any()


# ----------------------------------------------------------------------------------------------------------- B. special values
def test_special_values():
    st, prop, sse, expect = special_case()
    C = len(SPECIAL)
    D = _upload(st, prop=prop, sse=sse)
    _mcmc_accept(D, 1.0, C, CHAIN0, 3, 3, SEED, 1)
    _check_state(D, accept_np(st, prop, sse, 1.0, 0, CHAIN0, SEED, 1), "special")
    alphas, nacc, best = D.get("alphas")[:, 2], D.get("nacc"), D.get("best")
    for b, (take, alpha) in enumerate(expect):
        assert nacc[b] == int(take) and same(alphas[b], np.float64(alpha)), SPECIAL[b]
    assert bits(alphas[1:2])[0] == 0                                                  # exactly +0
    assert same(best[4], prop[4]) and D.get("best_lp")[0, 4] == -1.0                  # a tie with the best: taken
    assert same(best[5], st["best"][5]) and D.get("best_lp")[0, 5] == 5.0             # below the best: untouched


# ------------------------------------------------------------------------------------------------------------- C. SSE parts
@pytest.mark.parametrize("nparts", NPARTS)
def test_sse_parts_are_added_left_to_right(nparts):
    st, prop, parts = parts_case(nparts)
    D = _upload(st, prop=prop, sse=parts)
    _mcmc_accept(D, 1.0, 2, CHAIN0, 3, 4, SEED, 0, nparts=nparts)
    lps = D.get("lps")[:, 3]
    for c in range(2):
        if nparts > 2:
            assert np.sum(parts[c]) != lsum(parts[c])                                 # the pairwise sum differs: the case can tell
        assert same(lps[c], np.float64(-0.5 * lsum(parts[c]))), (nparts, c, lps[c])
    _check_state(D, accept_np(st, prop, parts, 1.0, 0, CHAIN0, SEED, 0), f"parts {nparts}")


# --------------------------------------------------------------------------------------------- D. the HMC / tempered form
@pytest.mark.parametrize("beta", HMC_BETA)
@pytest.mark.parametrize("p", HMC_P)
def test_hmc_accept_direct(p, beta):
    _lib, L = _L()
    assert L.qn_hmc_parts(p) == hmc_parts(p)
    par, step = 1, 2
    st, q, gq, sse, kc, kp, bt = hmc_case(p, beta, par, step)
    want = accept_np(st, q, sse, 1.0, 0, CHAIN0, SEED, par, kin_cur=kc, kin_prop=kp, gprop=gq, beta=bt)
    ref = _alpha_ref(st, step, HMC_TARGET)
    more = dict(prop=q, sse=sse, gprop=gq, kin_cur=kc, kin_prop=kp, beta=bt)
    D = _upload(st, **more)
    _hmc_accept(D, 1.0, 3, CHAIN0, p, 4, SEED, par, True)
    _check_state(D, want, f"hmc_accept_t p={p} beta={beta}", ref)
    nacc, gc = D.get("nacc"), D.get("grad_cur")
    assert nacc[0] == 4 and nacc[1] == 4                                              # chain 0 accepted, chain 1 did not
    took = nacc - st["nacc"]
    for b in range(3):
        assert same(gc[b], gq[b] if took[b] else st["grad_cur"][b])
        nlp = -0.5 * sse[b, 0] if took[b] else st["cur_lp"][par, b]                  # untempered
        assert same(D.get("lps")[b, step + 1], np.float64(nlp)) and same(D.get("cur_lp")[1 - par, b], np.float64(nlp))
    assert same(D.get("best_lp")[1 - par], np.array([-0.5 * sse[0, 0], 0.0, 0.0]))
    # chain = NULL: everything else as before
    st_nc = {k: v for k, v in st.items() if k != "chain"}
    Dn = _upload(st_nc, **more)
    _hmc_accept(Dn, 1.0, 3, CHAIN0, p, 4, SEED, par, True)
    for k in STATE:
        if st_nc.get(k) is not None:
            assert same(Dn.get(k), D.get(k)), k
    if beta == 1.0:                                                                   # qn_hmc_accept == qn_hmc_accept_t at beta = 1
        D1 = _upload(st, **more)
        _hmc_accept(D1, 1.0, 3, CHAIN0, p, 4, SEED, par, False)
        for k in STATE:
            if st.get(k) is not None:
                assert same(D1.get(k), D.get(k)), k


# -------------------------------------------------------------------------------- E. six steps without the host in between
def test_six_steps_with_history_alternating_parity():
    st, props, sse = six_step_case()
    C, p = st["cur"].shape
    kcap, pstride = st["hist"].shape[1:]
    D = _upload(st)
    steps = [Dev(prop=props[t], sse=sse[t]) for t in range(6)]
    for t in range(6):
        D.t["prop"], D.t["sse"] = steps[t].t["prop"], steps[t].t["sse"]
        _mcmc_accept(D, 1.0, C, CHAIN0, p, 6, SEED, t & 1, kcap=kcap, pstride=pstride)
        st = accept_np(st, props[t], sse[t], 1.0, 0, CHAIN0, SEED, t & 1)
        _check_state(D, st, f"six steps, after step {t}")
        assert np.array_equal(D.get("alphas")[:, t + 1], [np.inf if SIX_PATTERN[c][t] == "A" else 0.0 for c in range(C)])
    assert np.array_equal(D.get("kcur")[0], [4, 2, 4]) and np.array_equal(D.get("mult"), [[1, 3, 1], [2, 3, 2], [1, 1, 1]])


# ---------------------------------------------------------------------------------------------- F. the fused next proposal
@pytest.mark.parametrize("c1", [0.0, 0.25])
@pytest.mark.parametrize("p", [5, 1031])
@pytest.mark.parametrize("mode", [1, 2])
def test_fused_next_proposal_equals_the_separate_kernel(mode, p, c1):
    """prop_next of qn_mcmc_accept_propose against qn_mcmc_propose (mode 1) / qn_mcmc_apply_delta (mode 2) called afterwards on
    the state the accept left, with the step counter it advanced.  The proposal's normals come from float32 device intrinsics
    (log2, sin, cos), which no host library reproduces bit for bit: the separate kernel is the only exact reference there is.
    (Its own draws are held to numpy in tests/test_gpu_hist_product.py.)  Chain 0 accepts, chain 1 rejects."""
    _lib, L = _L()
    TB = L.qn_mcmc_hist_block_steps()
    rs = np.random.RandomState(10 * p + mode)
    C, par, step, t_next, s_iso = 2, 1, 4, 7, 0.29
    st = new_state(dyadic(rs, (C, p)), [-1e300, -1.0], [-1e300, 5.0], step, par, 6)
    prop, sse = dyadic(rs, (C, p)), np.array([[2.0], [np.inf]])
    sd, delta = rs.uniform(0.1, 2.0, (C, p)), 3.0 * rs.randn(C, TB, p)
    D = _upload(st, prop=prop, sse=sse, sd=sd, delta=delta, prop_next=np.full((C, p), np.nan), sep=np.full((C, p), np.nan))
    _mcmc_accept(D, 1.0, C, CHAIN0, p, 6, SEED, par, nxt=(mode, c1, t_next, s_iso))
    want = accept_np(st, prop, sse, 1.0, 0, CHAIN0, SEED, par)
    _check_state(D, want, f"fused mode {mode}")
    assert same(D.get("cur")[0], prop[0]) and same(D.get("cur")[1], st["cur"][1])
    sp = D.ptr("step_ptr", 8 * (1 - par))                                             # the slot the accept wrote: step + 1
    if mode == 1:
        _lib.check(L.qn_mcmc_propose(D.ptr("cur"), D.ptr("sd"), c1, C, CHAIN0, p, SEED, sp, D.ptr("sep"), None), "propose")
    else:
        _lib.check(L.qn_mcmc_apply_delta(D.ptr("cur"), D.ptr("delta"), t_next, s_iso, C, CHAIN0, p, SEED, sp, D.ptr("sep"), None), "apply_delta")
    _sync()
    nxt, sep = D.get("prop_next"), D.get("sep")
    assert np.isfinite(nxt).all() and same(nxt, sep)
    assert not same(nxt, want["cur"]) and same(D.get("sd"), sd) and same(D.get("delta"), delta)


# ---------------------------------------------------------------------------------------------- G. leapfrog at the grid cap
def _eps_arg(D, d, C):
    return d["eps"] if np.ndim(d["eps"]) == 0 else D.ptr("eps")


def _begin(L, variant, D, d, C, p, step):
    a = (D.ptr("cur"), D.ptr("g"), d["sigma"])
    b = (C, CHAIN0, p, SEED, D.ptr("step"), D.ptr("mom"), D.ptr("q"), D.ptr("kin"), None)
    if variant == "fixed":
        return L.qn_hmc_begin(*a, float(d["eps"]), *b)
    if variant.startswith("s"):
        return L.qn_hmc_begin_s(*a, D.ptr("eps"), D.ptr("scale"), *b)
    return L.qn_hmc_begin_t(*a, D.ptr("eps"), D.ptr("scale"), D.ptr("beta"), *b)


def _leap(L, variant, D, d, dtype, last, C, p):
    b = (last, C, p, D.ptr("mom"), D.ptr("q"), D.ptr("kin"), None)
    if variant == "fixed":
        return L.qn_hmc_leap(D.ptr("g"), dtype, d["sigma"], float(d["eps"]), *b)
    if variant.startswith("s"):
        return L.qn_hmc_leap_s(D.ptr("g"), dtype, d["sigma"], D.ptr("eps"), D.ptr("scale"), *b)
    return L.qn_hmc_leap_t(D.ptr("g"), dtype, d["sigma"], D.ptr("eps"), D.ptr("scale"), D.ptr("beta"), *b)


def _draws(L, _lib, C, p, step):
    """the momentum draw z of (SEED, step, chains CHAIN0 ..): a begin call on a zero state with a zero gradient"""
    zero = np.zeros((C, p))
    D = Dev(cur=zero, g=zero, step=np.array([step, -1], dtype=np.int64), mom=np.full((C, p), np.nan), q=np.full((C, p), np.nan),
            kin=np.full((C, hmc_parts(p)), np.nan), nrm=np.full((C, p), np.nan))
    _lib.check(L.qn_hmc_begin(D.ptr("cur"), D.ptr("g"), 1.0, 0.5, C, CHAIN0, p, SEED, D.ptr("step"), D.ptr("mom"), D.ptr("q"), D.ptr("kin"), None),
               "qn_hmc_begin")
    _lib.check(L.qn_mcmc_propose(None, None, 0.0, C, CHAIN0, p, SEED, D.ptr("step"), D.ptr("nrm"), None), "qn_mcmc_propose")
    _sync()
    z = D.get("mom")
    assert np.isfinite(z).all() and same(z.astype(np.float32).astype(np.float64), z)  # 24-bit significands
    assert same(D.get("nrm"), z)                                                      # the elementwise normals of the step: same keys
    assert same(D.get("q"), 0.5 * z)
    return z, D.get("kin")


@pytest.mark.parametrize("variant", LEAP_VARIANTS)
@pytest.mark.parametrize("p", LEAP_P)
def test_leapfrog_bit_for_bit(p, variant):
    """begin and leap of every entry point at sizes on both sides of the 64-workgroup cap (p > 65536: more than one trip of a
    workgroup's loop), both gradient dtypes, inner and last call: mom, q and EACH kinetic partial sum equal the float64 model.
    That the model is exact on these inputs (every product exact, so the fma rounds as multiply + add does) is asserted."""
    _lib, L = _L()
    C, step = 2, 5
    assert L.qn_hmc_parts(p) == hmc_parts(p)
    z, kin0 = _draws(L, _lib, C, p, step)
    d = leap_case(p, variant, True)
    ks, es, ok = leap_factors(d["sigma"], d["eps"], 0, d["scale"], d["beta"], C)
    mom, q, kin = begin_np(d["q"], d["g"], z, d["sigma"], d["eps"], d["scale"], d["beta"])
    assert ok and products_exact((0.5 * ks, d["g"]), (es, mom))
    assert same(kin0, kin)                                                            # K_cur parts do not depend on eps / scale / beta
    nanp, nank = np.full((C, p), np.nan), np.full((C, hmc_parts(p)), np.nan)
    D = Dev(cur=d["q"], g=d["g"], eps=np.atleast_1d(d["eps"]), scale=d["scale"], beta=d["beta"], step=np.array([step, -1], dtype=np.int64),
            mom=nanp, q=nanp, kin=nank)
    _lib.check(_begin(L, variant, D, d, C, p, step), "begin")
    _sync()
    assert same(D.get("mom"), mom) and same(D.get("q"), q), ("begin", p, variant)
    got = D.get("kin")
    assert same(got, kin), ("begin kin_parts", p, variant, np.argwhere(bits(got) != bits(kin))[:4])
    for x in ("cur", "g"):
        assert same(D.get(x), d["q" if x == "cur" else "g"])
    d = leap_case(p, variant, False)
    for last in (0, 1):
        ks, es, ok = leap_factors(d["sigma"], d["eps"], last, d["scale"], d["beta"], C)
        m, qn, kin = leap_np(d["g"], d["mom"], d["q"], d["sigma"], d["eps"], last, d["scale"], d["beta"])
        ml, ql, kl = leap_np(d["g"], d["mom"], d["q"], d["sigma"], d["eps"], last, d["scale"], d["beta"], ft=LD)
        assert ok and products_exact((ks, d["g"]), (es, m), (m, m)) and np.array_equal(m.astype(LD), ml) and np.array_equal(qn.astype(LD), ql)
        assert kin is None or np.array_equal(kin.astype(LD), kl)                      # exact: any order of the sum gives it
        for dtype, npdt in ((_lib.QN_F64, np.float64), (_lib.QN_F32, np.float32)):
            qin = nanp if last else d["q"]                                            # the last call must neither read nor write q
            D = Dev(g=d["g"].astype(npdt), eps=np.atleast_1d(d["eps"]), scale=d["scale"], beta=d["beta"], mom=d["mom"], q=qin, kin=nank)
            _lib.check(_leap(L, variant, D, d, dtype, last, C, p), "leap")
            _sync()
            what = ("leap", p, variant, "last" if last else "inner", npdt.__name__)
            assert same(D.get("mom"), m), what
            assert same(D.get("q"), qin if last else qn), what
            got = D.get("kin")
            assert same(got, kin if last else nank), what + (np.argwhere(bits(got) != bits(kin if last else nank))[:4],)
            assert same(D.get("g"), d["g"].astype(npdt))


def test_leapfrog_general_inputs():
    """p = 70001 with inputs that are not dyadic (qn_hmc_leap_t: eps, scale and beta from the device), against longdouble:
    mom within 5 x 2^-53 x its largest intermediate (gs beta, f eps, their product, x scale, fma), q within 7 x (mom's five,
    eps x scale, fma), each partial sum within (n + 2) 2^-53 sum(mom^2) of the longdouble sum of the DEVICE's momenta."""
    _lib, L = _L()
    rs = np.random.RandomState(70001)
    C, p, sigma = 2, 70001, 0.3
    eps, beta = np.array([0.0123, 0.0457]), np.array([0.37, 0.81])
    scale, g, mom, q = rs.uniform(0.5, 2.0, (C, p)), 40.0 * rs.randn(C, p), rs.randn(C, p), 0.5 * rs.randn(C, p)
    u = LD(2.0) ** -53
    for last in (0, 1):
        D = Dev(g=g, eps=eps, scale=scale, beta=beta, mom=mom, q=q, kin=np.full((C, hmc_parts(p)), np.nan))
        _lib.check(L.qn_hmc_leap_t(D.ptr("g"), _lib.QN_F64, sigma, D.ptr("eps"), D.ptr("scale"), D.ptr("beta"), last, C, p, D.ptr("mom"),
                                   D.ptr("q"), D.ptr("kin"), None), "qn_hmc_leap_t")
        _sync()
        ml, ql, _ = leap_np(g, mom, q, sigma, eps, last, scale, beta, ft=LD)
        kick = LD(0.5 if last else 1.0) * eps.astype(LD)[:, None] * (LD(-0.5) / (LD(sigma) * LD(sigma)) * beta.astype(LD)[:, None])
        big_m = np.maximum(np.maximum(np.abs(mom), np.abs(kick * scale * g)), np.abs(ml))
        r_m = float((np.abs(D.get("mom").astype(LD) - ml) / (5 * u * big_m)).max())
        print(f"\nstep_kernels leap general last={last}: mom err/bar = {r_m:.3f}")
        assert r_m <= 1.0
        if last:
            assert same(D.get("q"), q)
            dm2 = np.square(D.get("mom").astype(LD))
            r_k = max(float(abs(LD(D.get("kin")[c, k]) - dm2[c, lo:hi].sum()) / ((hi - lo + 2) * u * dm2[c, lo:hi].sum()))
                      for c in range(C) for k, (lo, hi) in enumerate(part_ranges(p, False)))
            print(f"step_kernels leap general last=1: kin_parts err/bar = {r_k:.3f}")
            assert r_k <= 1.0
        else:
            es = eps.astype(LD)[:, None] * scale
            big_q = np.maximum(np.maximum(np.abs(q), np.abs(es) * big_m), np.abs(ql))
            r_q = float((np.abs(D.get("q").astype(LD) - ql) / (7 * u * big_q)).max())
            print(f"step_kernels leap general last=0: q err/bar = {r_q:.3f}")
            assert r_q <= 1.0 and same(D.get("kin"), np.full((C, hmc_parts(p)), np.nan))
