"""NUTS warm-up with per-chain diagonal mass windows: the contract of qn_nuts_adapt (csrc/qn_nuts_adapt.hip;
include/quinn_amd_nuts_adapt.h) and of `DeviceNUTS(adapt_mass=True)`, restated in float64 numpy on top of `nuts.nuts_iter` and
`adapt.warmup_plan(adapt, True)`.  Build-only: the reference has no such sampler.

The chains of `quinn_amd.mcmc.nuts` run on their own step counters, so the windowed warm-up of `quinn_amd.mcmc.adapt` -- which
the host plans per launch for lock-step chains (qn_hmc_adapt) -- is looked up per CHAIN here: a table `plan` with one row per
warm-up step k = 1 .. adapt (m, the index of the step in the current dual-averaging run; n, the states collected in the current
window; collect / finish / freeze), read at the chain's own k.  `nuts_iter` runs with adapt = 0 -- its own dual averaging uses m =
t + 1 and cannot restart at a window end -- and `nuts_warm_update` follows every iteration.

A chain ENDED A STEP in an iteration iff t of the state the iteration wrote is t + 1 of the state it read; k is the new value,
the number of completed steps.  For such a chain with k <= adapt and s = plan[k - 1]:

    a = alphas[k], NaN counted as 0, capped at 1
    dual averaging: `adapt.HostAdaptation.update` with m = s['m'] on ws = (mu, hbar, logbar); eps = exp(logeps), or exp(logbar)
        when s['freeze']
    collect:  d = x - mean; mean += d / n; m2 += d (x - mean)                with x = cur (the row just stored), n = s['n']
    finish:   scale = sqrt((n / (n + 5)) m2 / (n - 1) + 1e-3 * 5 / (n + 5)); mean = m2 = 0; mu = log(10 eps); hbar = logbar = 0
    if k < nmcmc the next step has started (n_leap == 0) and its first half kick and drift used the old eps and scale: they
        are redone from the edge, u = ul + (hk scale) gl, q = ql + (dr scale) u with hk = v ((eps / 2) gs), dr = v eps, the new
        values and the v of the new step.  ul (= z), rho, the parts of |z|^2 and H0 stay: the momenta are whitened, z and
        |z|^2 / 2 do not depend on the scale.
    the state's eps becomes eps.

A chain that ended no step, a chain with k > adapt and a done chain are not touched; their ws is carried over.

Without windows (adapt < 20: no row of the plan has finish) nothing restarts and m = k throughout: the update is then
`nuts.dual_average` itself, in its operations, and `nuts_run_adapted` equals `nuts.nuts_run` bit for bit -- the path the device
engine takes in that case (qn_nuts_iter's own averaging).  With windows the operations are `HostAdaptation.update`'s, which
differ from `nuts.dual_average`'s in the last bit (a division where that one multiplies by a reciprocal).
"""
import numpy as np

from .adapt import GAMMA, KAPPA, T0, warmup_plan
from .nuts import _kick_drift, dual_average, normals, nuts_config, nuts_init, nuts_iter

PLAN_COLLECT, PLAN_FINISH, PLAN_FREEZE = 1, 2, 4           # the flag bits of the device's plan table


def plan_table(adapt):
    """`warmup_plan(adapt, True)` as the int32 table [adapt, 4] qn_nuts_adapt reads: m, n, flags (PLAN_*), 0."""
    rows = [(s['m'], s['n'], PLAN_COLLECT * s['collect'] + PLAN_FINISH * s['finish'] + PLAN_FREEZE * s['freeze'], 0)
            for s in warmup_plan(int(adapt), True)]
    return np.array(rows, dtype=np.int32).reshape(-1, 4)


def has_windows(plan):
    return any(s['finish'] for s in plan)


def warm_state(eps0, p):
    """ws at the start of a run: mu = log(10 eps0), hbar = logbar = 0 and empty moments."""
    return {'mu': np.log(10 * np.float64(eps0)), 'hbar': np.float64(0.0), 'logbar': np.float64(0.0),
            'mean': np.zeros(p), 'm2': np.zeros(p)}


def nuts_warm_update(st_old, st_new, ws, cfg, plan, alphas_row, given=None):
    """The warm-up update of ONE chain after an iteration that read st_old and wrote st_new (`nuts.nuts_iter` with adapt = 0).
    ws: dict(mu, hbar, logbar, mean [p], m2 [p]); cfg: the chain's constants, cfg['adapt'] the warm-up steps and cfg['scale']
    the current scale; plan: `warmup_plan(cfg['adapt'], True)`; alphas_row [nmcmc + 1]: the chain's acceptance statistics.
    given: {'eps': ..., 'mu': ..., 'hbar': ..., 'logbar': ...} -- the scalars as the caller's exp / log / pow formed them,
    taken in place of this file's (the device's, so that everything elementwise can be compared bit for bit).
    Nothing is written in place.  Returns (st, ws, cfg): the arguments themselves for a chain that is not touched."""
    k = st_new['t']
    if k != st_old['t'] + 1 or k > cfg['adapt'] or k < 1:
        return st_new, ws, cfg
    s, given = plan[k - 1], given or {}
    a = alphas_row[k]
    ws = dict(ws)
    if has_windows(plan):                                  # `HostAdaptation.update`, operation by operation
        m = s['m']
        a = np.where(np.isnan(a), 0.0, np.minimum(1.0, a))
        ws['hbar'] = (1 - 1 / (m + T0)) * ws['hbar'] + (cfg['target'] - a) / (m + T0)
        logeps = ws['mu'] - np.sqrt(m) / GAMMA * ws['hbar']
        eta = m ** -KAPPA
        ws['logbar'] = eta * logeps + (1 - eta) * ws['logbar']
        eps = np.exp(ws['logbar'] if s['freeze'] else logeps)
    else:                                                  # `nuts.dual_average`: m = k, frozen at k == adapt
        da = {'t': k - 1, 'mu': float(ws['mu']), 'hbar': float(ws['hbar']), 'logbar': float(ws['logbar'])}
        dual_average(da, cfg, a)
        ws['hbar'], ws['logbar'], eps = np.float64(da['hbar']), np.float64(da['logbar']), da['eps']
    ws['hbar'], ws['logbar'] = (np.float64(given.get(key, ws[key])) for key in ('hbar', 'logbar'))
    eps = np.float64(given.get('eps', eps))
    if s['collect']:
        n = s['n']
        d = st_new['cur'] - ws['mean']
        ws['mean'] = ws['mean'] + d / n
        ws['m2'] = ws['m2'] + d * (st_new['cur'] - ws['mean'])
    if s['finish']:
        n = s['n']
        cfg = dict(cfg, scale=np.sqrt((n / (n + 5)) * ws['m2'] / (n - 1) + 1e-3 * 5 / (n + 5)))
        ws['mean'], ws['m2'] = np.zeros_like(ws['mean']), np.zeros_like(ws['m2'])
        ws['mu'] = np.float64(given.get('mu', np.log(10 * eps)))
        ws['hbar'], ws['logbar'] = np.float64(0.0), np.float64(0.0)
    st = dict(st_new, eps=float(eps))
    if k < cfg['nmcmc']:                                   # the next step has started: its first half kick and drift again
        st['q'], st['u'] = _kick_drift(cfg, st['eps'], st['v'], st['ql'], st['ul'], st['gl'])
    return st, ws, cfg


def nuts_run_adapted(lp_and_grad, cur0, epsilon, nmcmc, max_depth=10, adapt=0, target_accept=0.8, seed=0, chain=0, scale=None,
                     warm=None):
    """`nuts.nuts_run` with the warm-up of this file: `nuts_iter` with adapt = 0, `nuts_warm_update` behind it.  Returns
    nuts_run's dict plus 'mass_scale' [p] (the scale at the end: the given one, or 1, where no window finished) and 'ws'.
    warm: a list that receives (k, alpha, cur, state, ws, cfg) after the update of every warm-up step k."""
    cfg = nuts_config(1.0, 0, nmcmc, max_depth, adapt, target_accept, seed, chain, scale, gs=1.0, const=0.0)
    plan = warmup_plan(cfg['adapt'], True)
    cur = np.array(cur0, dtype=np.float64)
    p = cur.size
    lp0, g0 = lp_and_grad(cur)
    st = nuts_init(cur, lp0, g0, epsilon, cfg, normals(seed, 0, chain, p))
    ws = warm_state(epsilon, p)
    out = {'chain': np.empty((nmcmc + 1, p)), 'lps': np.empty(nmcmc + 1), 'alphas': np.zeros(nmcmc + 1),
           'depth': np.zeros(nmcmc + 1, dtype=np.int32), 'nleap': np.zeros(nmcmc + 1, dtype=np.int32)}
    out['chain'][0], out['lps'][0] = cur, st['lp_cur']
    while st['t'] < nmcmc:
        lp, g = lp_and_grad(st['q'])
        old = st
        st, _ = nuts_iter(old, lp, g, dict(cfg, adapt=0))
        if 'row' in st:
            r, row, lpr, al, dep, nl = st['row']
            out['chain'][r], out['lps'][r], out['alphas'][r], out['depth'][r], out['nleap'][r] = row, lpr, al, dep, nl
        new = st
        st, ws, cfg = nuts_warm_update(old, new, ws, cfg, plan, out['alphas'])
        if warm is not None and st is not new:
            warm.append((st['t'], out['alphas'][st['t']], st['cur'], st, ws, cfg))
    out.update(ndiv=st['ndiv'], ntreedepth=st['ntreedepth'], ngrad=st['ngrad'], epsilon=st['eps'], best=st['best'],
               best_lp=st['best_lp'], mass_scale=np.broadcast_to(np.asarray(cfg['scale'], dtype=np.float64), (p,)).copy(), ws=ws)
    return out
