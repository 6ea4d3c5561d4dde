"""Warm-up adaptation of HMC / MALA: per-chain step size by dual averaging, per-chain diagonal mass by windowed Welford moments.

One contract for the host samplers (`HMC`, `MALA`; numpy, this file) and the device engines (`DeviceHMC`, `DeviceMALA`;
the _s leapfrog of csrc/qn_hmc_leap.hip, qn_hmc_adapt of csrc/qn_hmc_adapt.hip).  Chain c carries a step size eps_c and a positive per-parameter scale s[c, :] (square
root of the inverse mass, 1 at the start); the leapfrog runs in whitened momenta u = s * r:

    z ~ N(0, I);  u = z + (eps_c/2) s*g(cur);  q = cur + eps_c s*u
    L-1 times:    u += eps_c s*g(q);  q += eps_c s*u
    last:         u += (eps_c/2) s*g(q);        K_cur = sum z^2 / 2,  K_prop = sum u^2 / 2

with the sampler's usual accept rule (MALA is L = 1).  Step size: dual averaging of Hoffman & Gelman 2014 (algorithm 5)
with Stan's constants.  After the m-th warm-up step of the current run, a = min(1, mh) (NaN counts as 0):

    Hbar = (1 - 1/(m+t0)) Hbar + (delta - a)/(m+t0);   logeps = mu - sqrt(m)/gamma * Hbar
    logbar = m^-kappa logeps + (1 - m^-kappa) logbar;   the next step uses exp(logeps)

from mu = log(10 eps0), Hbar = logbar = 0; after the last warm-up step eps_c = exp(logbar), frozen from then on.  Mass:
inside the slow windows of `warmup_schedule` the post-accept state feeds n += 1; d = x - mean; mean += d/n;
M2 += d*(x - mean); at a window end s = sqrt((n/(n+5)) M2/(n-1) + 1e-3 * 5/(n+5)), the moments are reset and dual
averaging restarts with mu = log(10 eps_c) (the step size just computed), Hbar = logbar = 0, m = 0.
"""
from collections import namedtuple

import numpy as np

GAMMA, T0, KAPPA = 0.05, 10.0, 0.75
TARGET_ACCEPT = {'hmc': 0.8, 'mala': 0.574}

WarmupSchedule = namedtuple('WarmupSchedule', ['start', 'ends'])
WarmupSchedule.__doc__ = """start: warm-up steps before the first slow window (steps start + 1 .. ends[-1], counted from 1,
feed the moments); ends: the steps after which a window closes.  No window: start = nwarm, ends = ()."""


def warmup_schedule(nwarm):
    """Stan's windowed warm-up: initial buffer 75, terminal buffer 50, slow windows from 25 steps doubling, the last one
    stretched to the terminal buffer; 15 % / 75 % / 10 % if 75 + 25 + 50 > nwarm; no window (step size only) if nwarm < 20.
    warmup_schedule(300).ends == (100, 150, 250); warmup_schedule(1000).ends == (100, 150, 250, 450, 950)."""
    nwarm = int(nwarm)
    if nwarm < 20:
        return WarmupSchedule(max(nwarm, 0), ())
    init, term, base = 75, 50, 25
    if init + base + term > nwarm:
        init, term = int(0.15 * nwarm), int(0.1 * nwarm)
        base = nwarm - (init + term)
    last = nwarm - term
    ends, end, size = [], init + base, base
    while True:
        ends.append(end)
        if end == last:
            break
        size *= 2
        end += size
        if end - 1 + 2 * size >= last:                  # the window after this one would not fit: stretch this one
            end = last
    return WarmupSchedule(init, tuple(ends))


def warmup_plan(nwarm, adapt_mass=True):
    """Per warm-up step k = 1 .. nwarm the launch arguments of the adaptation: a list of dicts with m (index of the step in
    the current dual-averaging run), collect, finish, freeze and n (states collected in the current window, this one
    included; 0 outside the windows)."""
    sched = warmup_schedule(nwarm) if adapt_mass else WarmupSchedule(nwarm, ())
    ends = set(sched.ends)
    plan, m, n = [], 0, 0
    for k in range(1, nwarm + 1):
        m += 1
        collect = bool(sched.ends) and sched.start < k <= sched.ends[-1]
        n = n + 1 if collect else 0
        finish = k in ends
        plan.append({'m': m, 'collect': collect, 'finish': finish, 'freeze': k == nwarm, 'n': n})
        if finish:
            m, n = 0, 0
    return plan


def check_adapt_args(adapt, target_accept, nmcmc=None):
    adapt = int(adapt)
    if adapt < 0:
        raise ValueError("adapt is the number of warm-up steps (>= 0)")
    if adapt and not 0.0 < float(target_accept) < 1.0:
        raise ValueError("target_accept must lie in (0, 1)")
    if nmcmc is not None and adapt > nmcmc:
        raise ValueError(f"adapt = {adapt} warm-up steps exceed nmcmc = {nmcmc}")
    return adapt


class HostAdaptation:
    """The contract in numpy for C chains of p parameters: `eps` (C,), `scale` (C, p) (None without windows), and
    `update(k, mh, cur)` after the accept decision of warm-up step k = 1 .. nwarm."""

    def __init__(self, C, p, eps0, nwarm, target_accept, adapt_mass=True):
        self.nwarm, self.delta = int(nwarm), float(target_accept)
        self.plan = warmup_plan(self.nwarm, adapt_mass)
        self.eps = np.full(C, float(eps0))
        self.mu = np.log(10 * self.eps)
        self.hbar, self.logbar = np.zeros(C), np.zeros(C)
        self.has_mass = any(s['finish'] for s in self.plan)
        self.scale = np.ones((C, p)) if self.has_mass else None
        self.mean, self.m2 = np.zeros((C, p)), np.zeros((C, p))

    def update(self, k, mh, cur):
        s = self.plan[k - 1]
        m = s['m']
        a = np.where(np.isnan(mh), 0.0, np.minimum(1.0, mh))
        self.hbar = (1 - 1 / (m + T0)) * self.hbar + (self.delta - a) / (m + T0)
        logeps = self.mu - np.sqrt(m) / GAMMA * self.hbar
        eta = m ** -KAPPA
        self.logbar = eta * logeps + (1 - eta) * self.logbar
        self.eps = np.exp(self.logbar if s['freeze'] else logeps)
        if s['collect']:
            n = s['n']
            d = cur - self.mean
            self.mean = self.mean + d / n
            self.m2 = self.m2 + d * (cur - self.mean)
        if s['finish']:
            n = s['n']
            self.scale = np.sqrt((n / (n + 5)) * self.m2 / (n - 1) + 1e-3 * 5 / (n + 5))
            self.mean, self.m2 = np.zeros_like(self.mean), np.zeros_like(self.m2)
            self.mu = np.log(10 * self.eps)
            self.hbar, self.logbar = np.zeros_like(self.hbar), np.zeros_like(self.logbar)
