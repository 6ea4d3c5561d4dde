"""Replica exchange (parallel tempering; Swendsen & Wang 1986, Geyer 1991) for the device HMC / MALA engines: the contract of
qn_hmc_begin_t / qn_hmc_leap_t / qn_hmc_accept_t / qn_pt_swap (csrc/qn_hmc_leap.hip, qn_mcmc.hip, qn_temper.hip; include/quinn_amd.h), restated in numpy.

The C lock-step chains are K = C / R ladders of R rungs, ladder-major: chain c is rung c % R of ladder c // R and samples
pi(w)^beta_r with 1 = beta_0 > ... > beta_{R-1} > 0.  A rung's HMC step is the untempered one with the force beta_r * d logpost and
the potential beta_r * U in the accept test; every stored log-posterior stays untempered.  After every `swap_every`-th step an
exchange round follows: round k pairs the chains (c, c + 1) with c % R in {e, e + 2, ...}, e = k & 1 (deterministic even-odd
scheme, Okabe et al. 2001), and a pair swaps its states iff

    u < exp((beta_c - beta_{c+1}) * (lp_{c+1} - lp_c)),      u = `swap_uniform(seed, t, global id of c)`, t the step just decided

with lp the untempered log-posteriors (a NaN or infinite lp never moves).  Each rung's chain leaves pi^beta_r invariant under
both moves, so the cold chains (rung 0) sample the target itself while inheriting the hot rungs' barrier crossings.

beta scales the whole log-posterior: the likelihood alone by default, where hot rungs of a network with flat directions can wander
far, or likelihood and prior with `priorsigma` (`quinn_amd.mcmc.prior`: a hot rung's prior then has the bounded variance
priorsigma^2 / beta); `beta_min` is the caller's choice.  Not here: ladder adaptation, tempering of
AMCMC and of the SG samplers, host engines, thermodynamic integration.
"""
import numpy as np

from .sgmcmc import ctr_of, philox4x32

PURPOSE_SWAP = 6


def ladder(R, beta_min=0.01):
    """float64 [R], the inverse temperatures of one ladder.  R an int >= 2: geometric, beta_r = beta_min ** (r / (R - 1)) with
    0 < beta_min < 1.  R a sequence: taken as it is; it must start at 1 and decrease strictly to a positive value."""
    if np.ndim(R) == 0:
        if isinstance(R, (bool, np.bool_)) or int(R) != R or int(R) < 2:
            raise ValueError(f"ladder = {R!r}: a ladder has >= 2 rungs (an int R or a decreasing sequence of beta starting at 1)")
        if not 0.0 < float(beta_min) < 1.0:
            raise ValueError(f"beta_min = {beta_min!r}: must lie in (0, 1)")
        R = int(R)
        beta = float(beta_min) ** (np.arange(R) / (R - 1))
        beta[0], beta[-1] = 1.0, float(beta_min)
        return beta
    beta = np.asarray(R, dtype=np.float64)
    if beta.ndim != 1 or beta.size < 2:
        raise ValueError("ladder: a sequence of >= 2 inverse temperatures")
    if beta[0] != 1.0 or not np.all(np.diff(beta) < 0) or not beta[-1] > 0.0:
        raise ValueError("ladder: the inverse temperatures start at 1 and decrease strictly to a positive value")
    return beta.copy()


def swap_pairs(R, round):
    """The lower rungs r of the pairs (r, r + 1) of exchange round `round`: e, e + 2, ... with e = round & 1 and r + 1 < R."""
    return list(range(int(round) & 1, int(R) - 1, 2))


def swap_uniform(seed, t, chain):
    """The uniform in (0, 1) (53 bits) that decides the swap of GLOBAL chain `chain` (the pair's lower chain; scalar or array)
    with its upper neighbour after step t: words 0 and 1 of the Philox block (seed, stream 2 t + 1, ctr_of(chain, 6, 0)) --
    bit for bit the kernel's."""
    ch = np.asarray(chain, dtype=np.uint64)
    w = philox4x32(seed, 2 * int(t) + 1, ctr_of(ch, PURPOSE_SWAP, np.zeros_like(ch)))
    bits = (w[..., 0].astype(np.uint64) << np.uint64(21)) ^ (w[..., 1].astype(np.uint64) >> np.uint64(11))
    return (bits.astype(np.float64) + 0.5) * (1.0 / 9007199254740992.0)


def swap_round(lp, beta, R, round, u):
    """One exchange round on C = len(lp) ladder-major chains.  lp [C]: untempered log-posteriors; beta [C]; u [C]: the uniform of
    every chain (read at the lower chain of each pair).  Returns (swapped, perm): swapped [C] bool, True at the lower chain of
    every pair that exchanges; perm [C], the chain slot whose state chain c holds afterwards (new[c] = old[perm[c]])."""
    lp, beta, u = (np.asarray(v, dtype=np.float64) for v in (lp, beta, u))
    C, R = lp.shape[0], int(R)
    if C % R:
        raise ValueError(f"{C} chains are not whole ladders of {R} rungs")
    swapped, perm = np.zeros(C, dtype=bool), np.arange(C)
    for k in range(C // R):
        for r in swap_pairs(R, round):
            c = k * R + r
            d = (beta[c] - beta[c + 1]) * (lp[c + 1] - lp[c])
            with np.errstate(over='ignore', invalid='ignore'):
                if np.isfinite(lp[c]) and np.isfinite(lp[c + 1]) and u[c] < np.exp(d):
                    swapped[c] = True
                    perm[c], perm[c + 1] = c + 1, c
    return swapped, perm


def check_whole_ladders(R, C=None, chain0=0):
    """Refuses chains that are not whole ladders of R rungs: C chains (None: unknown) starting at GLOBAL chain chain0."""
    if int(chain0) % R:
        raise ValueError(f"chain0 = {chain0} is not a ladder boundary (R = {R}): groups and rank shards must hold whole ladders")
    if C is not None and int(C) % R:
        raise ValueError(f"{C} chains are not whole ladders of R = {R} rungs: the number of chains (of every group and rank "
                         "shard) must be a multiple of R")


def check_temper_args(ladder_arg, beta_min=0.01, swap_every=1, C=None, chain0=0, use_graph=False):
    """Refuses what the tempered engines cannot run; returns the ladder's beta [R].  C / chain0 (when known): the chains of an
    engine, a group or a rank shard must be whole ladders."""
    beta = ladder(ladder_arg, beta_min)
    if isinstance(swap_every, (bool, np.bool_)) or int(swap_every) != swap_every or int(swap_every) < 1:
        raise ValueError(f"swap_every = {swap_every!r}: an exchange round follows every swap_every-th step, swap_every >= 1")
    if use_graph:
        raise ValueError("ladder with use_graph=True: the exchange rounds break the captured two-step unit; run a ladder "
                         "with use_graph=False")
    check_whole_ladders(beta.size, C, chain0)
    return beta


def round_trips(rep, R):
    """int [C]: per replica the number of completed tours rung 0 -> rung R - 1 -> rung 0, from the replica trace rep
    [C, nrounds + 1] (rep[c, k]: the replica in chain slot c after k exchange rounds; replicas are numbered like the slots they
    start in, up to a common offset)."""
    rep = np.asarray(rep)
    C, R = rep.shape[0], int(R)
    ids = rep[:, 0]
    pos = {int(v): i for i, v in enumerate(ids)}
    trips = np.zeros(C, dtype=np.int64)
    state = np.zeros(C, dtype=np.int8)          # 0: not yet at rung 0; 1: left rung 0, heading up; 2: reached the top, heading down
    rung = np.arange(C) % R
    for k in range(rep.shape[1]):
        for c in range(C):
            i = pos[int(rep[c, k])]
            if rung[c] == 0:
                if state[i] == 2:
                    trips[i] += 1
                state[i] = 1
            elif rung[c] == R - 1 and state[i] == 1:
                state[i] = 2
    return trips
