"""CPU: the contract of NUTS's windowed warm-up (`quinn_amd.mcmc.nuts_adapt`) -- per chain it is `HostAdaptation` fed with the
chain's own steps, without windows it is `nuts.nuts_run`'s dual averaging bit for bit, the redone half kick and drift is exact,
the adapted scale shortens the trajectories of an ill-scaled Gaussian, and the kernel's header is bound."""
import ctypes
import re

import numpy as np
import pytest

from quinn_amd import _lib
from quinn_amd.mcmc import nuts
from quinn_amd.mcmc import nuts_adapt as na
from quinn_amd.mcmc.adapt import HostAdaptation, warmup_plan, warmup_schedule

PREC3 = np.array([1.0, 16.0, 0.25])


def gauss3(q):
    return -0.5 * float(np.sum(PREC3 * q * q)), -PREC3 * q


SD8 = np.array([1.0, 0.01] * 4)                       # the ill-scaled Gaussian: standard deviations alternating 1 and 0.01


def gauss8(q):
    return -0.5 * float(np.sum((q / SD8) ** 2)), -q / SD8 ** 2


def run3(adapt, nmcmc, **kw):
    warm = []
    out = na.nuts_run_adapted(gauss3, np.array([0.3, -0.1, 0.5]), 0.3, nmcmc, max_depth=5, adapt=adapt, seed=11, chain=2,
                              warm=warm, **kw)
    return out, warm


@pytest.mark.parametrize("adapt,nmcmc", [(40, 48), (300, 310)])
def test_a_chain_is_host_adaptation_fed_with_its_own_steps(adapt, nmcmc):
    """`HostAdaptation.update` on the (alpha, cur) of the chain's warm-up steps, in their order: the same eps, mu, hbar, logbar,
    mean, m2 and scale after EVERY step, bit for bit.  adapt = 40 has one window (steps 7 .. 36), adapt = 300 three."""
    assert warmup_schedule(40) == (6, (36,)) and warmup_schedule(300).ends == (100, 150, 250)
    out, warm = run3(adapt, nmcmc)
    assert [w[0] for w in warm] == list(range(1, adapt + 1))
    host = HostAdaptation(1, 3, 0.3, adapt, 0.8)
    for k, alpha, cur, st, ws, cfg in warm:
        assert alpha == out['alphas'][k] and np.array_equal(cur, out['chain'][k])
        host.update(k, np.array([alpha]), cur[None])
        assert st['eps'] == host.eps[0], k
        assert (ws['mu'], ws['hbar'], ws['logbar']) == (host.mu[0], host.hbar[0], host.logbar[0]), k
        assert np.array_equal(ws['mean'], host.mean[0]) and np.array_equal(ws['m2'], host.m2[0]), k
        assert np.array_equal(np.broadcast_to(cfg['scale'], (3,)), host.scale[0]), k
    assert out['epsilon'] == host.eps[0] and np.array_equal(out['mass_scale'], host.scale[0])
    assert not np.array_equal(out['mass_scale'], np.ones(3))
    # the scale is that of the target, roughly (a window of 30 or 100 correlated states): within a factor 2.5
    assert np.all(np.abs(np.log(out['mass_scale'] * np.sqrt(PREC3))) < np.log(2.5))


def test_without_windows_it_is_nuts_run():
    """adapt = 12 has no window: every array and scalar of `nuts.nuts_run(adapt=12)`, bit for bit."""
    assert warmup_schedule(12).ends == () and not na.has_windows(warmup_plan(12, True))
    out, warm = run3(12, 30)
    ref = nuts.nuts_run(gauss3, np.array([0.3, -0.1, 0.5]), 0.3, 30, max_depth=5, adapt=12, seed=11, chain=2)
    assert len(warm) == 12
    for k in ('chain', 'lps', 'alphas', 'depth', 'nleap', 'best'):
        assert np.array_equal(out[k], ref[k]), k
    for k in ('ndiv', 'ntreedepth', 'ngrad', 'epsilon', 'best_lp'):
        assert out[k] == ref[k], k
    assert np.array_equal(out['mass_scale'], np.ones(3))
    sc = np.array([0.9, 0.3, 1.7])                                                  # a handed-over scale is kept
    out, _ = run3(12, 20, scale=sc)
    ref = nuts.nuts_run(gauss3, np.array([0.3, -0.1, 0.5]), 0.3, 20, max_depth=5, adapt=12, seed=11, chain=2, scale=sc)
    assert np.array_equal(out['chain'], ref['chain']) and np.array_equal(out['mass_scale'], sc)


def test_the_redo_is_exact():
    """After a window end: q, u are `_kick_drift` from the edge (ql, ul, gl) with the new eps and scale; ul, rho, H0 are those of
    the untouched state; and the energy error of the step's first leaf is that of a direct evaluation of the Hamiltonian
    H(q, r) = -lp(q) + |scale r|^2 / 2 along one leapfrog in the momentum r = u / scale."""
    nmcmc, adapt = 48, 40
    cfg = nuts.nuts_config(1.0, 0, nmcmc, 5, adapt, 0.8, 11, 2, None, gs=1.0, const=0.0)
    plan = warmup_plan(adapt, True)
    cur = np.array([0.3, -0.1, 0.5])
    st = nuts.nuts_init(cur, *gauss3(cur), 0.3, cfg, nuts.normals(11, 0, 2, 3))
    ws, alphas, seen = na.warm_state(0.3, 3), np.zeros(nmcmc + 1), 0
    while st['t'] < nmcmc:
        old = st
        new, _ = nuts.nuts_iter(old, *gauss3(old['q']), dict(cfg, adapt=0))
        if 'row' in new:
            alphas[new['row'][0]] = new['row'][3]
        st, ws, cfg2 = na.nuts_warm_update(old, new, ws, cfg, plan, alphas)
        if st is new:
            assert ws is not None and cfg2 is cfg                                   # not touched: the arguments themselves
            continue
        k = st['t']
        assert k <= adapt and st['n_leap'] == 0
        q, u = nuts._kick_drift(cfg2, st['eps'], st['v'], st['ql'], st['ul'], st['gl'])
        assert np.array_equal(st['q'], q) and np.array_equal(st['u'], u)
        for key in ('ul', 'ur', 'rho', 'ql', 'gl', 'cur', 'gcur'):
            assert st[key] is new[key], key
        assert st['H0'] == new['H0'] and st['v'] == new['v']
        if plan[k - 1]['finish']:
            assert k == 36 and not np.array_equal(cfg2['scale'], cfg['scale'])
            assert not np.array_equal(st['q'], new['q'])
        # ---- the first leaf of step k, directly: H in (q, r), r = z / scale, one leapfrog of size v eps
        s, eps, v, z = np.broadcast_to(cfg2['scale'], (3,)), st['eps'], st['v'], st['ul']
        r0 = z / s
        lp0, g0 = gauss3(st['cur'])
        rh = r0 + (0.5 * v * eps) * g0
        q1 = st['cur'] + (v * eps) * s * s * rh
        lp1, g1 = gauss3(q1)
        r1 = rh + (0.5 * v * eps) * g1
        dE = (-lp1 + 0.5 * np.sum((s * r1) ** 2)) - (-lp0 + 0.5 * np.sum((s * r0) ** 2))
        nxt, _ = nuts.nuts_iter(st, *gauss3(st['q']), dict(cfg2, adapt=0))
        assert np.allclose(st['q'], q1, rtol=1e-13, atol=1e-15)
        if dE <= nuts.DIVERGENCE:
            got = -nxt['logW_sub']                                 # (leaf 0 of a subtree sets logW_sub = -dE; a step's end keeps it)
            # a difference of energies of size ~|lp|: 1e-12 of them is thousands of ulp, and far below any effect of a
            # kick or drift made with the old eps or scale (which changes dE in its leading digits)
            assert abs(got - dE) <= 1e-12 * (1 + abs(lp0) + abs(lp1)), (k, got, dE)
        cfg = cfg2
        seen += 1
    assert seen == adapt


# mean leapfrogs per step after warm-up, measured with this file (seed 3, chain 0): unit mass 208.7, with windows 6.4 (step sizes 0.011 and 0.64)
def test_windows_shorten_the_trajectories_of_an_ill_scaled_gaussian():
    """p = 8, standard deviations alternating 1 and 0.01, adapt = 300, 200 further steps, max_depth = 8.  The leapfrogs of a
    step grow with the ratio of the largest to the smallest scale: about 100 at unit mass, single digits when whitened.
    Required: the mean nleap after warm-up with unit mass is at least 4 times that with windows."""
    q0 = SD8 * np.array([0.5, -1.0, 1.5, 0.3, -0.7, 1.1, -0.2, 0.8])
    unit = nuts.nuts_run(gauss8, q0, 0.01, 500, max_depth=8, adapt=300, seed=3)
    wind = na.nuts_run_adapted(gauss8, q0, 0.01, 500, max_depth=8, adapt=300, seed=3)
    nl_unit, nl_wind = unit['nleap'][301:].mean(), wind['nleap'][301:].mean()
    print(f"mean nleap after warm-up: unit mass {nl_unit:.1f}, with windows {nl_wind:.1f}; eps {unit['epsilon']:.3g} / "
          f"{wind['epsilon']:.3g}; scale {wind['mass_scale']}")
    assert nl_unit >= 4 * nl_wind
    assert np.all(np.abs(np.log(wind['mass_scale'] / SD8)) < np.log(2.0))             # the scale found is the target's


def test_plan_table_is_warmup_plan():
    for adapt in (1, 12, 40, 300):
        tab, plan = na.plan_table(adapt), warmup_plan(adapt, True)
        assert tab.shape == (adapt, 4) and tab.dtype == np.int32
        for row, s in zip(tab, plan):
            assert (row[0], row[1]) == (s['m'], s['n']) and row[3] == 0
            assert (bool(row[2] & na.PLAN_COLLECT), bool(row[2] & na.PLAN_FINISH), bool(row[2] & na.PLAN_FREEZE)) == \
                (s['collect'], s['finish'], s['freeze'])


def test_header_is_bound_and_exported():
    _lib.build()
    L = _lib.lib()
    hdr = open(_lib.NUTS_ADAPT_HEADER).read()
    funcs, consts = _lib.parse_header(hdr)
    assert funcs == _lib.NUTS_ADAPT_FUNCTIONS and list(funcs) == ["qn_nuts_adapt"]
    code = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    assert set(re.findall(r"\b(qn_[a-z_0-9]+)\s*\(", code)) == set(funcs)
    others = set(_lib.FUNCTIONS) | set(_lib.PSIS_FUNCTIONS) | set(_lib.STACK_FUNCTIONS) | set(_lib.RANK_FUNCTIONS) | \
        set(_lib.EV_FUNCTIONS) | set(_lib.QUANT_FUNCTIONS)
    assert not set(funcs) & others
    assert len(_lib.FUNCTIONS) == 72 and "qn_nuts_adapt.hip" in _lib.SOURCES
    assert consts == {"QN_NUTS_PLAN_COLLECT": na.PLAN_COLLECT, "QN_NUTS_PLAN_FINISH": na.PLAN_FINISH,
                      "QN_NUTS_PLAN_FREEZE": na.PLAN_FREEZE}
    vp, i32, i64, f64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double
    assert funcs["qn_nuts_adapt"] == (i32, [vp, vp, i32, i32, f64, vp, vp, vp, i32, i32, i64, f64] + [vp] * 10)
    fn = L.qn_nuts_adapt
    assert (fn.restype, list(fn.argtypes)) == funcs["qn_nuts_adapt"]


def adapt_abi_args(**over):
    """Arguments of qn_nuts_adapt with every pointer a non-NULL dummy that a refused call never touches."""
    a = dict(cur=8, alphas=8, nmcmc=10, adapt=5, target_accept=0.8, plan=8, es=8, ei=8, parity=0, C=2, p=3, sigma=0.5, ql=8,
             ul=8, gl=8, q=8, u=8, ws=8, mean=8, m2=8, scale=8, stream=None)
    a.update(over)
    return list(a.values())


PTRS = ('cur', 'alphas', 'plan', 'es', 'ei', 'ql', 'ul', 'gl', 'q', 'u', 'ws', 'mean', 'm2', 'scale')
REFUSED = [{'C': 0}, {'C': 65536}, {'p': 0}, {'sigma': 0.0}, {'sigma': float('nan')}, {'nmcmc': 0}, {'adapt': 0}, {'adapt': 11},
           {'parity': 2}, {'parity': -1}, {'target_accept': 0.0}, {'target_accept': 1.0}] + [{k: None} for k in PTRS]


@pytest.mark.parametrize("over", REFUSED, ids=lambda o: "%s=%s" % next(iter(o.items())))
def test_refusals_need_no_device(over):
    _lib.build()
    L = _lib.lib()
    assert L.qn_nuts_adapt(*adapt_abi_args(**over)) == _lib.CONSTANTS["QN_EINVAL"]
    assert L.qn_last_error().decode().startswith("qn_nuts_adapt:")


def test_engine_refusals_need_no_device():
    from quinn_amd.mcmc.device_nuts import DeviceNUTS
    ok = dict(epsilon=0.05, adapt=40, adapt_mass=True)
    assert DeviceNUTS.check_params((2, 8, 1), 'float64', 48, None, **ok)['nuts_adapt_mass'] is True
    assert DeviceNUTS.check_params((2, 8, 1), 'float64', 48, None, epsilon=0.05, adapt=40)['nuts_adapt_mass'] is False
    for bad in (dict(ok, adapt=0), dict(ok, adapt_mass=1), dict(ok, adapt_mass='yes'), dict(ok, use_graph=True),
                dict(ok, ladder=[1.0, 0.5]), dict(ok, adapt=49)):
        with pytest.raises(ValueError):
            DeviceNUTS.check_params((2, 8, 1), 'float64', 48, None, **bad)
