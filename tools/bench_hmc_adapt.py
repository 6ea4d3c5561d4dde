#!/usr/bin/env python3
"""Device HMC warm-up at cfg2 (64 chains, 3x64 tanh, N = 4096, L = 3) on one MI355X; writes profiles/hmc_adapt.txt (--out).

  1. cost of reading eps / scale from device arrays: steps/s of the fixed-step engine (qn_hmc_begin / qn_hmc_leap, adapt=0)
     against the same chain on qn_hmc_begin_s / qn_hmc_leap_s with eps [C] frozen at the same value, without and with a
     scale array of ones; the three are timed alternately, `--rounds` times, in one process (median and minimum);
  2. steps/s of the warm-up phase (every step followed by qn_hmc_adapt), with and without mass windows;
  3. ESS per second of the log-posterior trace (qn_chain_stats over all chains, rows after the warm-up) of the adapted run
     against the hand-searched step size of profiles/r04_hmc_mala_device_end_to_end.json, each at its own sampling rate.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from quinn_amd.mcmc import diagnostics as diag              # noqa: E402
from quinn_amd.mcmc.device_hmc import DeviceHMC             # noqa: E402
from quinn_amd.ops import BatchedMLP, MLPArch               # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hmc_adapt.txt"))
ap.add_argument("--steps", type=int, default=600)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--nwarm", type=int, default=1000)
ap.add_argument("--nsamp", type=int, default=2000)
args = ap.parse_args()
assert torch.cuda.is_available(), "needs the MI355X"

SIGMA, L, C, N = 0.02, 3, 64, 4096
arch = MLPArch((1, 64, 64, 64, 1), "tanh")
rs = np.random.RandomState(0)
x = rs.rand(N, 1) * 2 * np.pi - np.pi
y = 0.02 * rs.randn(N, 1) + np.sin(x)
op = BatchedMLP(arch, x, y)
ini = np.stack([0.1 * np.random.RandomState(1000 + c).randn(arch.nparams) for c in range(C)])
with open(os.path.join(ROOT, "profiles", "r04_hmc_mala_device_end_to_end.json")) as f:
    hand_eps = json.loads([ln for ln in f if ln.startswith("{")][0])["cfg2"]["epsilon"]


class Frozen(DeviceHMC):
    """The _s kernels at a fixed step size: one warm-up step whose adaptation is replaced by writing the step size back
    (and, with ones=True, a scale array of ones), so that everything after it runs on the frozen device arrays."""
    ones = False

    def _adapt_step(self, s, nmcmc, a):
        s['eps'].fill_(self.epsilon)
        if self.ones:
            s['scale'] = torch.ones_like(s['cur'])


def timed(eng, nsteps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = eng.run(nsteps, ini, store_chain=False)
    torch.cuda.synchronize()
    return nsteps / (time.perf_counter() - t0), r


lines = [f"# tools/bench_hmc_adapt.py: cfg2, {C} chains, 3x64 tanh, N = {N}, L = {L}, sigma = {SIGMA}, float64, one MI355X",
         f"# hand-searched step size (profiles/r04_hmc_mala_device_end_to_end.json): {hand_eps:.6g}"]

# ---- 1. fixed-step kernels against the _s kernels at the same step size
engines = {"fixed (adapt=0)": DeviceHMC(op, SIGMA, epsilon=hand_eps, L=L, seed=1),
           "_s, eps [C]": Frozen(op, SIGMA, epsilon=hand_eps, L=L, seed=1, adapt=1, adapt_mass=False),
           "_s, eps [C] + scale of ones": Frozen(op, SIGMA, epsilon=hand_eps, L=L, seed=1, adapt=1, adapt_mass=False)}
engines["_s, eps [C] + scale of ones"].ones = True
rates = {k: [] for k in engines}
for k, e in engines.items():
    timed(e, 100)                                           # code objects, clock
ref_lp = None
for _ in range(args.rounds):
    for k, e in engines.items():
        rate, r = timed(e, args.steps)
        rates[k].append(rate)
        if ref_lp is None:
            ref_lp = r['logpost']
        # step 0 of the Frozen engines is a warm-up step at the same step size: the whole chain must be the fixed engine's
        assert torch.equal(r['logpost'], ref_lp), k
lines.append(f"## sampling phase, {args.steps} steps, {args.rounds} alternating rounds (identical chains, bit for bit): steps/s median / min / max")
base = statistics.median(rates["fixed (adapt=0)"])
for k, v in rates.items():
    lines.append(f"{k:32s} {statistics.median(v):9.1f} {min(v):9.1f} {max(v):9.1f}   x{statistics.median(v) / base:.4f} of fixed")

# ---- 2. warm-up phase
lines.append(f"## warm-up phase, {args.nwarm} steps (every step followed by qn_hmc_adapt): steps/s")
for mass in (False, True):
    e = DeviceHMC(op, SIGMA, epsilon=hand_eps, L=L, seed=1, adapt=args.nwarm, adapt_mass=mass)
    timed(e, args.nwarm)
    v = [timed(e, args.nwarm)[0] for _ in range(3)]
    lines.append(f"adapt_mass={mass!s:5s} {statistics.median(v):9.1f} {min(v):9.1f} {max(v):9.1f}")

# ---- 3. effective samples per second of the log-posterior trace
lines.append(f"## ESS of the log-posterior trace over {C} chains, rows after {args.nwarm}, {args.nsamp} sampling steps")
nm = args.nwarm + args.nsamp
runs = {"hand-searched, fixed": (DeviceHMC(op, SIGMA, epsilon=hand_eps, L=L, seed=1), base),
        "adapted from 10 x hand-searched": (DeviceHMC(op, SIGMA, epsilon=10 * hand_eps, L=L, seed=1, adapt=args.nwarm),
                                            statistics.median(rates["_s, eps [C] + scale of ones"])),
        "adapted, step size only": (DeviceHMC(op, SIGMA, epsilon=10 * hand_eps, L=L, seed=1, adapt=args.nwarm, adapt_mass=False),
                                    statistics.median(rates["_s, eps [C]"]))}
for k, (e, rate) in runs.items():
    r = e.run(nm, ini, store_chain=False)
    d = diag.diagnose_chains(r['logpost'][..., None].contiguous(), args.nwarm)
    ess, rhat = float(d['ess'][0]), float(d['rhat'][0])
    acc = float((r['logpost'][:, args.nwarm + 1:] != r['logpost'][:, args.nwarm:-1]).double().mean())
    eps = r['epsilon'].cpu().numpy() if 'epsilon' in r else np.full(C, hand_eps)
    lines.append(f"{k:32s} ESS {ess:9.1f}  R-hat {rhat:7.3f}  acceptance {acc:.3f}  epsilon {eps.min():.3g} .. {eps.max():.3g}  "
                 f"mean logpost {float(r['logpost'][:, args.nwarm:].mean()):.1f}  "
                 f"ESS/s {ess / (args.nsamp / rate):9.1f} (at {rate:.0f} steps/s)")
text = "\n".join(lines) + "\n"
print(text)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(text)
