"""The No-U-Turn sampler (Hoffman & Gelman 2014) in its multinomial form (Betancourt 2017) with asynchronous chain steps: the
contract of the device engine `DeviceNUTS` (qn_nuts_begin / qn_nuts_iter, csrc/qn_nuts.hip; include/quinn_amd.h), restated in
float64 numpy.  Build-only: the reference has no such sampler.

A step doubles a trajectory forwards or backwards in time until it turns back on itself; there is no trajectory length to
choose.  The ITERATIVE form runs here and on the device: one leapfrog, that is one gradient call, per iteration, and every
U-turn test of the binary tree is made from O(depth) stored checkpoints.  `nuts_step_recursive` is the textbook recursion, kept
only to pin the iterative form (tests/test_nuts_contract.py): the recursion is the authority.

Whitened momenta u = s r (s = `scale`, the square root of the inverse diagonal mass; 1 without): u ~ N(0, I), kinetic energy
|u|^2 / 2, every U-turn test a plain dot product -- the momenta of qn_hmc_begin_s (`quinn_amd.mcmc.adapt`).  The target enters
as sse(w) and g(w) = d sse / d w with lp = gs sse - lik_const and force gs g (gs = -0.5 / sigma^2; a prior is folded into both
beforehand: `quinn_amd.mcmc.prior`).  With hk = v ((eps / 2) gs) and dr = v eps, every product rounded once, no contraction:

    leapfrog in direction v = +-1 from a node (q, u, g):   u_half = u + (hk s) g;   q' = q + (dr s) u_half;
                                                           the gradient call at q' (the PENDING point);   u' = u_half + (hk s) g'

Per-chain state: the tree's proposal cur with its gradient gcur, sse_cur and lp_cur -- at a step's start and end the chain's
current point (nothing else of the old point is needed during a step: H0 is a scalar, the edges are copies); the two edges
(ql, ul, gl), (qr, ur, gr); rho (sum of the tree's momenta); of the subtree being built rho_sub, its proposal (sub_q, sub_g,
sse_sub, lp_sub), logW_sub and the checkpoints ck_u, ck_rho [max_depth, p]; the pending point q with the half-kicked momentum
u; the scalars eps, (mu, hbar, logbar) of dual averaging, H0, logW, sum_a and the counters t (the chain's OWN step), d
(doublings merged), i (leaf of the subtree), v, n_leap, ndiv, ntreedepth, ngrad; best, best_lp.

Start of step t (`nuts_begin`): z ~ N(0, I), H0 = -lp_cur + |z|^2 / 2; both edges = (cur, z, gcur), rho = z, logW = 0, d = i =
n_leap = 0, sum_a = 0; v = the direction of doubling 0; u = z + (hk s) gcur, q = cur + (dr s) u.

One iteration (`nuts_iter`), given sse' and g' at the pending point: leaf i of the subtree of doubling d (2^d leaves)
    u' = u + (hk s) g';  rho_sub = (i == 0 ? u' : rho_sub + u');  dE = (-lp' + |u'|^2 / 2) - H0, NaN counted as +inf
    a = min(1, exp(-dE)); sum_a += a; n_leap += 1; ngrad += 1;  the leaf is DIVERGENT iff dE > 1000: the step ends
    logW_sub = (i == 0 ? -dE : logaddexp(logW_sub, -dE));  with probability exp(-dE - logW_sub) the leaf becomes the subtree's
        proposal (uniform within the subtree: reservoir sampling in leaf order)
    i even and i + 1 < 2^d:  ck_u[idx_max] = u', ck_rho[idx_max] = rho_sub              idx_max = popcount(i >> 1)
    i odd:  for k = idx_max .. idx_min, r = (rho_sub - ck_rho[k]) + ck_u[k] (the sum of the momenta from the checkpoint's leaf
        to this one): the subtree TURNS iff r . ck_u[k] <= 0 or r . u' <= 0     idx_min = idx_max - (trailing one bits of i) + 1
        and the step ends.  These are the tests of every aligned sub-subtree of 2, 4, ... leaves that ends at leaf i.
    i + 1 < 2^d: the next leapfrog starts from the leaf, i += 1
    i + 1 == 2^d, the subtree is complete: with probability min(1, exp(logW_sub - logW)) (biased progressive sampling) the
        tree's proposal becomes the subtree's; logW = logaddexp(logW, logW_sub); rho += rho_sub; the edge on side v becomes
        the leaf; d += 1; the step ends if rho . ul <= 0 or rho . ur <= 0, or else if d == max_depth (counted in ntreedepth);
        otherwise a new direction is drawn and leaf 0 of the next subtree starts from that side's edge
This is the classic criterion on the whole tree and on every subtree, WITHOUT the extra checks across adjacent subtrees that
Stan added later (2.21); trajectories can therefore be one doubling longer than Stan's on some targets, the sampler stays exact.
A subtree that diverges or turns is discarded: the proposal, rho and the edges keep what the earlier doublings made of them.

Step end: row t + 1 of chain (= cur), lps (= lp_cur), alphas (= sum_a / n_leap), depth (the doublings started: d, or d + 1 when
the step ended inside a subtree) and nleap; ndiv += divergent; best <- cur where lp_cur >= best_lp; if t < adapt the step size
is dual-averaged with the constants and the formula of `quinn_amd.mcmc.adapt` on a = sum_a / n_leap with m = t + 1, and frozen
to exp(logbar) at t == adapt - 1 (step size only; the warm-up with mass windows runs with adapt = 0 here and
`quinn_amd.mcmc.nuts_adapt` behind every iteration); t += 1 and, if t < nmcmc, the next step starts in the same iteration.  A chain with t == nmcmc is done: none of its
arrays is read or written.

Random numbers: Philox4x32-10 keyed by (seed, stream = the chain's step t, [global chain id : 24][purpose : 4][index : 36]).
Purpose 9: the momenta, index = column pair (the device uses the float32-transcendental normals of the HMC momenta; `normals`
here is their float64 form, equal to ~1e-6).  Purpose 10: the scalar uniforms, index (kind << 32) | n -- kind 0 the direction
of doubling n (v = +1 iff u < 0.5), kind 1 the merge of doubling n, kind 2 the leaf whose n_leap was n before the increment.
"""
import math

import numpy as np

from .adapt import GAMMA, KAPPA, T0
from .ess import lik_const
from .sgmcmc import ctr_of, philox4x32

PURPOSE_MOM, PURPOSE_UNIF = 9, 10
KIND_DIR, KIND_MERGE, KIND_LEAF = 0, 1, 2
MAX_DEPTH_LIMIT = 12
DIVERGENCE = 1000.0
ES_KEYS = ('eps', 'mu', 'hbar', 'logbar', 'H0', 'logW', 'logW_sub', 'sum_a', 'sse_cur', 'lp_cur', 'sse_sub', 'lp_sub')  # es [2, C, 12]
EI_KEYS = ('t', 'd', 'i', 'v', 'n_leap', 'ndiv', 'ntreedepth', 'ngrad')                                               # ei [2, C, 8]
VEC_KEYS = ('cur', 'gcur', 'ql', 'ul', 'gl', 'qr', 'ur', 'gr', 'rho', 'rho_sub', 'sub_q', 'sub_g', 'q', 'u')
NDOT = 3 + 2 * MAX_DEPTH_LIMIT           # partial-sum slots per workgroup: |u'|^2, two per checkpoint, two of the tree


def _philox_words(seed, stream, ctr):
    """Philox4x32-10 of one counter in Python integers (`sgmcmc.philox4x32` for a scalar, without array overhead)."""
    M = 0xFFFFFFFF
    c0, c1, c2, c3 = ctr & M, (ctr >> 32) & M, stream & M, (stream >> 32) & M
    k0, k1 = seed & M, (seed >> 32) & M
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M, (p0 >> 32) ^ c3 ^ k1, p0 & M
        k0, k1 = (k0 + 0x9E3779B9) & M, (k1 + 0xBB67AE85) & M
    return c0, c1, c2, c3


def nuts_uniform(seed, t, chain, kind, n):
    """The scalar uniform (kind, n) of GLOBAL chain `chain` at its step t: u01 of words (0, 1) of the block (seed, stream t,
    ctr_of(chain, 10, (kind << 32) | n)), the device's bit for bit."""
    ctr = (int(chain) << 40) | (PURPOSE_UNIF << 36) | (((int(kind) << 32) | int(n)) & 0xFFFFFFFFF)
    w = _philox_words(int(seed), int(t), ctr)
    return (float((w[0] << 21) ^ (w[1] >> 11)) + 0.5) * (1.0 / 9007199254740992.0)


def normals(seed, t, chain, p):
    """z [p] of GLOBAL chain `chain` at its step t in float64: Box-Muller on the block (seed, t, ctr_of(chain, 9, column pair))
    with the device's bit layout (csrc/qn_mcmc_shared.h, normal2).  The device forms radius and angle with the hardware float32
    log2 / sin / cos: its momenta equal these to ~1e-6 of the radius, not bit for bit."""
    npair = (int(p) + 1) // 2
    w = philox4x32(seed, int(t), ctr_of(np.uint64(chain), PURPOSE_MOM, np.arange(npair, dtype=np.uint64))).astype(np.uint64)
    hi = w[:, 0] >> np.uint64(8)
    u1 = np.where(hi > 0, (hi.astype(np.float64) + 0.5) / 16777216.0,
                  ((w[:, 1] >> np.uint64(8)).astype(np.float64) + 0.5) / 16777216.0 / 16777216.0)
    u2 = (w[:, 2] >> np.uint64(8)).astype(np.float64) / 16777216.0
    r = np.sqrt(-2.0 * np.log(u1))
    z = np.stack([r * np.cos(2.0 * np.pi * u2), r * np.sin(2.0 * np.pi * u2)], axis=1).reshape(-1)
    return z[:int(p)]


def checkpoint_range(i):
    """(idx_min, idx_max) of leaf i: the checkpoint an even leaf writes is idx_max; an odd leaf tests idx_max down to idx_min."""
    idx_max = bin(i >> 1).count('1')
    ones = 0
    while (i >> ones) & 1:
        ones += 1
    return idx_max - ones + 1, idx_max


def logaddexp(a, b):
    """log(exp(a) + exp(b)) as the kernel forms it: max + log1p(exp(-|a - b|)); an infinite or NaN difference gives max."""
    hi, lo = (a, b) if a >= b else (b, a)
    d = lo - hi
    if not d > -math.inf:                                 # (-inf, or NaN from inf - inf)
        return hi
    return hi + math.log1p(math.exp(d))


def _exp(x):
    try:
        return math.exp(x)
    except OverflowError:
        return math.inf


def nuts_config(sigma, n_rows, nmcmc, max_depth=10, adapt=0, target_accept=0.8, seed=0, chain=0, scale=None, gs=None, const=None):
    """The constants of a run of ONE chain (`chain`: its global id), as the kernels take them."""
    return {'gs': -0.5 / (float(sigma) * float(sigma)) if gs is None else float(gs),
            'lik_const': float(lik_const(n_rows, sigma)) if const is None else float(const),
            'nmcmc': int(nmcmc), 'max_depth': int(max_depth), 'adapt': int(adapt), 'target': float(target_accept),
            'seed': int(seed), 'chain': int(chain), 'scale': 1.0 if scale is None else np.asarray(scale, dtype=np.float64)}


def _kick_drift(cfg, eps, v, q, u, g):
    """(q', u_half) of the first half of a leapfrog from the node (q, u, g)."""
    hk = v * ((0.5 * eps) * cfg['gs'])
    uh = u + (hk * cfg['scale']) * g
    return q + ((v * eps) * cfg['scale']) * uh, uh


def nuts_begin(st, cfg, z, zz=None):
    """Start of step st['t'] of ONE chain from (cur, gcur, lp_cur) with the momenta z [p]: the tree state, in place in the dict.
    zz: |z|^2 as the caller sums it (None: numpy's sum)."""
    z = np.array(z, dtype=np.float64)
    st['H0'] = -st['lp_cur'] + 0.5 * (float(np.sum(z * z)) if zz is None else float(zz))
    st['ql'] = st['qr'] = st['cur']
    st['ul'] = st['ur'] = st['rho'] = z
    st['gl'] = st['gr'] = st['gcur']
    st.update(logW=0.0, d=0, i=0, n_leap=0, sum_a=0.0)
    st['v'] = 1 if nuts_uniform(cfg['seed'], st['t'], cfg['chain'], KIND_DIR, 0) < 0.5 else -1
    st['q'], st['u'] = _kick_drift(cfg, st['eps'], st['v'], st['cur'], z, st['gcur'])
    return st


def nuts_init(cur, sse_cur, gcur, eps, cfg, z, max_depth=None):
    """The state after `qn_nuts_begin`: step 0 of one chain started from cur with SSE sse_cur and gradient gcur = d sse / d w."""
    cur, gcur = np.array(cur, dtype=np.float64), np.array(gcur, dtype=np.float64)
    p, D = cur.size, cfg['max_depth'] if max_depth is None else max_depth
    lp = cfg['gs'] * float(sse_cur) - cfg['lik_const']
    st = {'cur': cur, 'gcur': gcur, 'sse_cur': float(sse_cur), 'lp_cur': lp, 'eps': float(eps), 'mu': math.log(10.0 * float(eps)),
          'hbar': 0.0, 'logbar': 0.0, 'logW_sub': 0.0, 'sse_sub': 0.0, 'lp_sub': 0.0, 't': 0, 'ndiv': 0, 'ntreedepth': 0, 'ngrad': 0,
          'rho_sub': np.zeros(p), 'sub_q': np.zeros(p), 'sub_g': np.zeros(p), 'ck_u': np.zeros((D, p)), 'ck_rho': np.zeros((D, p)),
          'best': cur, 'best_lp': lp}
    return nuts_begin(st, cfg, z)


def dual_average(st, cfg, a):
    """The step size after warm-up step m = t + 1 with acceptance statistic a (`quinn_amd.mcmc.adapt`); frozen at the last."""
    m = st['t'] + 1
    a = min(1.0, a) if a == a else 0.0
    w = 1.0 / (m + T0)
    st['hbar'] = (1.0 - w) * st['hbar'] + (cfg['target'] - a) * w
    logeps = st['mu'] - (math.sqrt(m) / GAMMA) * st['hbar']
    eta = float(m) ** -KAPPA
    st['logbar'] = eta * logeps + (1.0 - eta) * st['logbar']
    st['eps'] = _exp(st['logbar'] if m == cfg['adapt'] else logeps)


def nuts_iter(st, sse, grad, cfg, z_next=None, dots=None, zz_next=None, eps_next=None):
    """One iteration of ONE chain: the SSE `sse` and the gradient `grad` [p] = d sse / d w of the pending point st['q'] have
    arrived.  st is left alone, a new dict is returned (arrays are replaced, never written in place).  z_next: the momenta of
    step t + 1 (read when a next step starts; None: `normals`), zz_next their sum of squares as the caller sums it, eps_next the
    adapted step size as the caller's exp / pow formed it (read after a warm-up step; None: this file's).  dots: the
    reduced quantities as the caller sums them (None: numpy's sums) -- {'uu': |u'|^2, 'ck': {k: (r . ck_u[k], r . u')},
    'tree': (rho . ul, rho . ur)}, the tree's with rho and the edges as they stand after the merge.
    Returns (state, event): 'done' | 'leaf' (the subtree goes on) | 'double' (a subtree was merged, the next one started) |
    'divergent' | 'turn_sub' | 'turn_tree' | 'max_depth' (the last four end the step: the state then carries 'row' = (t + 1,
    cur, lp_cur, alpha, depth, nleap)); st['leaf_selected'] / st['merged'] tell what this iteration's draws decided, and
    st['margin'] how close the closest of its decisions was to a tie (a dot product's distance from zero relative to the norms
    involved is not formed: the absolute value; a uniform's distance from its threshold; dE's from the divergence bound)."""
    st = {k: v for k, v in st.items() if k not in ('row', 'leaf_selected', 'merged', 'margin')}
    if st['t'] >= cfg['nmcmc']:
        return st, 'done'
    grad = np.asarray(grad, dtype=np.float64)
    seed, chain, t, d, i, v = cfg['seed'], cfg['chain'], st['t'], st['d'], st['i'], st['v']
    hk = v * ((0.5 * st['eps']) * cfg['gs'])
    u1 = st['u'] + (hk * cfg['scale']) * grad
    rs = u1 if i == 0 else st['rho_sub'] + u1
    st['u'], st['rho_sub'] = u1, rs
    complete = i + 1 == (1 << d)
    imin, imax = checkpoint_range(i)
    if i % 2 == 0 and not complete:
        st['ck_u'], st['ck_rho'] = st['ck_u'].copy(), st['ck_rho'].copy()
        st['ck_u'][imax], st['ck_rho'][imax] = u1, rs
    uu = float(np.sum(u1 * u1)) if dots is None else float(dots['uu'])
    lp1 = cfg['gs'] * float(sse) - cfg['lik_const']
    dE = (-lp1 + 0.5 * uu) - st['H0']
    if not dE == dE:
        dE = math.inf
    n0 = st['n_leap']
    st['sum_a'] += min(1.0, _exp(-dE))
    st['n_leap'] += 1
    st['ngrad'] += 1
    divergent = dE > DIVERGENCE
    turn = False
    st['leaf_selected'] = st['merged'] = False
    margin = [abs(dE - DIVERGENCE)]
    if not divergent:
        st['logW_sub'] = -dE if i == 0 else logaddexp(st['logW_sub'], -dE)
        margin.append(abs(nuts_uniform(seed, t, chain, KIND_LEAF, n0) - _exp(-dE - st['logW_sub'])))
        if nuts_uniform(seed, t, chain, KIND_LEAF, n0) < _exp(-dE - st['logW_sub']):
            st['leaf_selected'] = True
            st['sub_q'], st['sub_g'], st['sse_sub'], st['lp_sub'] = st['q'], grad, float(sse), lp1
        if i % 2 == 1:
            for k in range(imax, imin - 1, -1):
                if dots is None:
                    r = (rs - st['ck_rho'][k]) + st['ck_u'][k]
                    a, b = float(np.sum(r * st['ck_u'][k])), float(np.sum(r * u1))
                else:
                    a, b = dots['ck'][k]
                margin += [abs(a), abs(b)]
                turn = turn or a <= 0.0 or b <= 0.0
    st['margin'] = min(margin)
    if divergent or turn:
        event, depth = ('divergent' if divergent else 'turn_sub'), d + 1
    elif not complete:
        st['i'] = i + 1
        st['q'], st['u'] = _kick_drift(cfg, st['eps'], v, st['q'], u1, grad)
        return st, 'leaf'
    else:
        margin.append(abs(nuts_uniform(seed, t, chain, KIND_MERGE, d) - _exp(st['logW_sub'] - st['logW'])))
        if nuts_uniform(seed, t, chain, KIND_MERGE, d) < _exp(st['logW_sub'] - st['logW']):
            st['merged'] = True
            st['cur'], st['gcur'], st['sse_cur'], st['lp_cur'] = st['sub_q'], st['sub_g'], st['sse_sub'], st['lp_sub']
        st['logW'] = logaddexp(st['logW'], st['logW_sub'])
        rho = st['rho'] + rs
        ul, ur = (st['ul'], u1) if v > 0 else (u1, st['ur'])
        tl, tr = (float(np.sum(rho * ul)), float(np.sum(rho * ur))) if dots is None else dots['tree']
        st['d'] = d = d + 1
        depth = d
        st['margin'] = min(margin + [abs(tl), abs(tr)])
        if tl <= 0.0 or tr <= 0.0:
            event = 'turn_tree'
        elif d == cfg['max_depth']:
            event = 'max_depth'
            st['ntreedepth'] += 1
        else:                                                      # the tree goes on: merge the arrays, start the next subtree
            st['rho'] = rho
            if v > 0:
                st['qr'], st['ur'], st['gr'] = st['q'], u1, grad
            else:
                st['ql'], st['ul'], st['gl'] = st['q'], u1, grad
            st['v'] = v = 1 if nuts_uniform(seed, t, chain, KIND_DIR, d) < 0.5 else -1
            st['i'] = 0
            edge = (st['qr'], st['ur'], st['gr']) if v > 0 else (st['ql'], st['ul'], st['gl'])
            st['q'], st['u'] = _kick_drift(cfg, st['eps'], v, *edge)
            return st, 'double'
    # ---- the step ends
    alpha = st['sum_a'] / st['n_leap']
    st['row'] = (t + 1, st['cur'], st['lp_cur'], alpha, depth, st['n_leap'])
    st['ndiv'] += int(divergent)
    if st['lp_cur'] >= st['best_lp']:
        st['best'], st['best_lp'] = st['cur'], st['lp_cur']
    if t < cfg['adapt']:
        dual_average(st, cfg, alpha)
        if eps_next is not None:
            st['eps'] = float(eps_next)
    st['t'] = t + 1
    if st['t'] < cfg['nmcmc']:
        nuts_begin(st, cfg, normals(seed, st['t'], chain, st['cur'].size) if z_next is None else z_next, zz_next)
    return st, event


def nuts_run(lp_and_grad, cur0, epsilon, nmcmc, max_depth=10, adapt=0, target_accept=0.8, seed=0, chain=0, scale=None,
             trace=None):
    """One chain of nmcmc steps through `nuts_begin` / `nuts_iter` on a callable target lp_and_grad(q [p]) -> (log density,
    its gradient [p]) (the contract's sse and g with gs = 1 and no constant), with the Philox keys of (seed, chain): dict(chain
    [nmcmc + 1, p], lps, alphas [nmcmc + 1], depth, nleap [nmcmc + 1] int32, ndiv, ntreedepth, ngrad, epsilon).
    trace: a list that receives (t, event, pending point, leaf_selected, merged, margin) of every iteration."""
    cfg = nuts_config(1.0, 0, nmcmc, max_depth, adapt, target_accept, seed, chain, scale, gs=1.0, const=0.0)
    cur = np.array(cur0, dtype=np.float64)
    p = cur.size
    lp0, g0 = lp_and_grad(cur)
    st = nuts_init(cur, lp0, g0, epsilon, cfg, normals(seed, 0, chain, p))
    out = {'chain': np.empty((nmcmc + 1, p)), 'lps': np.empty(nmcmc + 1), 'alphas': np.zeros(nmcmc + 1),
           'depth': np.zeros(nmcmc + 1, dtype=np.int32), 'nleap': np.zeros(nmcmc + 1, dtype=np.int32)}
    out['chain'][0], out['lps'][0] = cur, st['lp_cur']
    while st['t'] < nmcmc:
        t, q = st['t'], st['q']
        lp, g = lp_and_grad(q)
        st, event = nuts_iter(st, lp, g, cfg)
        if trace is not None:
            trace.append((t, event, q, st['leaf_selected'], st['merged'], st['margin']))
        if 'row' in st:
            r, row, lpr, al, dep, nl = st['row']
            out['chain'][r], out['lps'][r], out['alphas'][r], out['depth'][r], out['nleap'][r] = row, lpr, al, dep, nl
    out.update(ndiv=st['ndiv'], ntreedepth=st['ntreedepth'], ngrad=st['ngrad'], epsilon=st['eps'], best=st['best'],
               best_lp=st['best_lp'])
    return out


def nuts_step_recursive(lp_and_grad, cur, lp_cur, g_cur, z, eps, max_depth, seed, t, chain, scale=None):
    """One step by the textbook RECURSION (Hoffman & Gelman 2014, algorithm 3 with Betancourt's multinomial weights): a subtree
    of depth j is two subtrees of depth j - 1 built one after the other, and it turns iff one of them does or its own summed
    momentum rho has rho . u_first <= 0 or rho . u_last <= 0.  It stops at the first leaf, in the order of the leapfrogs, that
    diverges or closes a turning subtree.  The draws are those of the iterative form, by their keys: the direction and the
    merge of doubling n, and per leaf the reservoir draw that makes the proposal uniform within the subtree.
    Returns dict(q, lp, leaves [list of points in leapfrog order], event, depth, nleap, sum_a, selected [leaf numbers that
    became a subtree's proposal], merged [doublings whose subtree was taken])."""
    cfg = nuts_config(1.0, 0, 1, max_depth, scale=scale, gs=1.0, const=0.0)
    z = np.asarray(z, dtype=np.float64)
    H0 = -lp_cur + 0.5 * float(np.sum(z * z))
    acc = {'leaves': [], 'sum_a': 0.0, 'selected': []}

    def leaf(node, v, sub):
        q, u, g = node
        q1, uh = _kick_drift(cfg, eps, v, q, u, g)
        lp1, g1 = lp_and_grad(q1)
        g1 = np.asarray(g1, dtype=np.float64)
        u1 = uh + ((v * ((0.5 * eps) * cfg['gs'])) * cfg['scale']) * g1
        dE = (-lp1 + 0.5 * float(np.sum(u1 * u1))) - H0
        if not dE == dE:
            dE = math.inf
        n0 = len(acc['leaves'])
        acc['leaves'].append(q1)
        acc['sum_a'] += min(1.0, _exp(-dE))
        if dE > DIVERGENCE:
            return None, 'divergent'
        sub['logW'] = -dE if sub['logW'] is None else logaddexp(sub['logW'], -dE)
        if nuts_uniform(seed, t, chain, KIND_LEAF, n0) < _exp(-dE - sub['logW']):
            sub['prop'] = (q1, lp1, g1)
            acc['selected'].append(n0)
        return {'first_u': u1, 'last': (q1, u1, g1), 'rho': u1}, None

    def build(node, v, depth, sub):
        if depth == 0:
            return leaf(node, v, sub)
        a, stop = build(node, v, depth - 1, sub)
        if stop:
            return None, stop
        b, stop = build(a['last'], v, depth - 1, sub)
        if stop:
            return None, stop
        rho = a['rho'] + b['rho']
        if float(np.sum(rho * a['first_u'])) <= 0.0 or float(np.sum(rho * b['last'][1])) <= 0.0:
            return None, 'turn_sub'
        return {'first_u': a['first_u'], 'last': b['last'], 'rho': rho}, None

    left = right = (np.asarray(cur, dtype=np.float64), z, np.asarray(g_cur, dtype=np.float64))
    rho, logW, prop, d, merged = z, 0.0, (left[0], lp_cur, left[2]), 0, []
    while True:
        v = 1 if nuts_uniform(seed, t, chain, KIND_DIR, d) < 0.5 else -1
        sub = {'logW': None, 'prop': None}
        res, stop = build(right if v > 0 else left, v, d, sub)
        if stop:
            event, depth = stop, d + 1
            break
        if nuts_uniform(seed, t, chain, KIND_MERGE, d) < _exp(sub['logW'] - logW):
            prop = sub['prop']
            merged.append(d)
        logW = logaddexp(logW, sub['logW'])
        rho = rho + res['rho']
        if v > 0:
            right = res['last']
        else:
            left = res['last']
        d += 1
        depth = d
        if float(np.sum(rho * left[1])) <= 0.0 or float(np.sum(rho * right[1])) <= 0.0:
            event = 'turn_tree'
            break
        if d == max_depth:
            event = 'max_depth'
            break
    return {'q': prop[0], 'lp': prop[1], 'leaves': acc['leaves'], 'event': event, 'depth': depth, 'nleap': len(acc['leaves']),
            'sum_a': acc['sum_a'], 'selected': acc['selected'], 'merged': merged}


def check_nuts_args(epsilon, max_depth=10, adapt=0, target_accept=0.8, block=32, nmcmc=None):
    """Refuses what the sampler cannot run; returns (epsilon as a float or a float64 array, max_depth, adapt, target_accept,
    block)."""
    if isinstance(epsilon, (bool, np.bool_, str)) or epsilon is None:
        raise ValueError(f"epsilon = {epsilon!r}: the step size is a number > 0 or an array of them, one per chain")
    eps = np.asarray(epsilon, dtype=np.float64)
    if eps.ndim > 1 or eps.size < 1 or not np.all(np.isfinite(eps)) or not np.all(eps > 0.0):
        raise ValueError(f"epsilon = {epsilon!r}: every step size must be > 0 and finite (a scalar or [C])")
    for name, val in (('max_depth', max_depth), ('adapt', adapt), ('block', block)):
        if isinstance(val, (bool, np.bool_)) or not isinstance(val, (int, np.integer)):
            raise ValueError(f"{name} = {val!r}: an integer")
    if not 1 <= int(max_depth) <= MAX_DEPTH_LIMIT:
        raise ValueError(f"max_depth = {max_depth!r}: 1 .. {MAX_DEPTH_LIMIT} doublings (a step makes at most 2^max_depth - 1 "
                         "gradient calls)")
    if int(adapt) < 0 or (nmcmc is not None and int(adapt) > int(nmcmc)):
        raise ValueError(f"adapt = {adapt!r}: the warm-up steps, 0 .. nmcmc" + ("" if nmcmc is None else f" = {int(nmcmc)}"))
    if not 1 <= int(block) <= 2 ** 20:
        raise ValueError(f"block = {block!r}: 1 .. 2^20 iterations between two looks at the step counters")
    if isinstance(target_accept, (bool, str)) or target_accept is None or not 0.0 < float(target_accept) < 1.0:
        raise ValueError(f"target_accept = {target_accept!r}: must lie in (0, 1)")
    return (float(eps) if eps.ndim == 0 else eps), int(max_depth), int(adapt), float(target_accept), int(block)
