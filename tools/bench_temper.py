#!/usr/bin/env python3
"""Replica exchange at cfg2 (64 chains, 3x64 tanh, N = 4096, HMC L = 3) on one MI355X; writes profiles/temper.txt (--out).

  1. qn_pt_swap alone: time per launch and achieved bytes/s (a swapping pair reads 4 p doubles and writes 4 p, plus the two
     rewritten chain rows), on states prepared so that every pair swaps, and so that none does;
  2. steps/s of the tempered engine (ladder of `--rungs`, an exchange round after every step) beside the same engine untempered,
     alternately in one process;
  3. split-R-hat of the log-posterior trace of the cold chains (64 / R of them) beside an untempered run of 64 / R chains with
     R times as many steps: the same total number of gradient evaluations.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from quinn_amd import _lib                                  # noqa: E402
from quinn_amd.mcmc import diagnostics as diag              # noqa: E402
from quinn_amd.mcmc import tempering as pt                  # noqa: E402
from quinn_amd.mcmc.device_hmc import DeviceHMC             # noqa: E402
from quinn_amd.ops import BatchedMLP, MLPArch               # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "temper.txt"))
ap.add_argument("--steps", type=int, default=400)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--rungs", type=int, default=8)
ap.add_argument("--beta-min", type=float, default=0.01)
ap.add_argument("--nwarm", type=int, default=300)
ap.add_argument("--nsamp", type=int, default=700)
ap.add_argument("--epsilon", type=float, default=2e-4)
args = ap.parse_args()
assert torch.cuda.is_available(), "needs the MI355X"

SIGMA, L, C, N, R = 0.02, 3, 64, 4096, args.rungs
arch = MLPArch((1, 64, 64, 64, 1), "tanh")
p = arch.nparams
rs = np.random.RandomState(0)
x = rs.rand(N, 1) * 2 * np.pi - np.pi
y = 0.02 * rs.randn(N, 1) + np.sin(x)
op = BatchedMLP(arch, x, y)
ini = np.stack([0.1 * np.random.RandomState(1000 + c).randn(p) for c in range(C)])
lines = [f"# tools/bench_temper.py: cfg2, {C} chains, 3x64 tanh (p = {p}), N = {N}, L = {L}, sigma = {SIGMA}, float64, one MI355X",
         f"# ladder: R = {R}, beta_min = {args.beta_min}, an exchange round after every step; epsilon = {args.epsilon}"]

# ---- 1. the swap launch alone
Lb = _lib.lib()
dev, f64 = "cuda", torch.float64
nm = 4
beta = torch.as_tensor(np.tile(pt.ladder(R, args.beta_min), C // R), dtype=f64, device=dev)
st = {'cur': torch.randn(C, p, dtype=f64, device=dev), 'g': torch.randn(C, p, dtype=f64, device=dev),
      'best_lp': torch.zeros(2, C, dtype=f64, device=dev), 'lps': torch.zeros(C, nm + 1, dtype=f64, device=dev),
      'chain': torch.zeros(C, nm + 1, p, dtype=f64, device=dev), 'rid': torch.zeros(2, C, dtype=torch.int32, device=dev),
      'rep': torch.zeros(C, 3, dtype=torch.int32, device=dev), 'acc': torch.zeros(C, dtype=torch.int64, device=dev),
      'try': torch.zeros(C, dtype=torch.int64, device=dev), 'step': torch.ones(2, dtype=torch.int64, device=dev)}
stream = _lib.stream()


def swap_time(cur_lp, nrep=200):
    lp2 = torch.stack([cur_lp, cur_lp])

    def go(k):
        _lib.check(Lb.qn_pt_swap(st['cur'].data_ptr(), st['g'].data_ptr(), lp2.data_ptr(), st['best_lp'].data_ptr(),
                                 st['lps'].data_ptr(), st['chain'].data_ptr(), beta.data_ptr(), st['rid'].data_ptr(),
                                 st['rep'].data_ptr(), st['acc'].data_ptr(), st['try'].data_ptr(), st['step'].data_ptr(), R, 0, 2,
                                 C, 0, p, nm, 1, 0, k & 1, stream), "qn_pt_swap")
    for k in range(20):
        go(k)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(nrep):
        go(k)                                               # (slot 0 is read every time: the same decision in every launch)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / nrep


rung = torch.arange(C, device=dev) % R
always = rung.double() * 1e6                               # hotter rungs hold the higher log-posterior: every pair swaps
never = -rung.double() * 1e6
npairs = (C // R) * len(pt.swap_pairs(R, 0))
lines.append(f"## qn_pt_swap alone, round 0 ({npairs} pairs of {C} chains), 200 back-to-back launches: time per launch")
for name, lp, moved in (("every pair swaps", always, npairs * 10 * p * 8), ("no pair swaps", never, npairs * 4 * p * 8)):
    ts = [swap_time(lp) for _ in range(3)]
    t = statistics.median(ts)
    lines.append(f"{name:20s} {t * 1e6:8.2f} us   {moved / t / 1e9:8.1f} GB/s ({moved / 1e6:.2f} MB read + written per launch)")


# ---- 2. steps/s beside the untempered engine
def timed(eng, nsteps, start):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = eng.run(nsteps, start, store_chain=False)
    torch.cuda.synchronize()
    return nsteps / (time.perf_counter() - t0), r


engines = {"untempered": DeviceHMC(op, SIGMA, epsilon=args.epsilon, L=L, seed=1),
           f"ladder R = {R}": DeviceHMC(op, SIGMA, epsilon=args.epsilon, L=L, seed=1, ladder=R, beta_min=args.beta_min)}
rates = {k: [] for k in engines}
for e in engines.values():
    timed(e, 50, ini)
for _ in range(args.rounds):
    for k, e in engines.items():
        rates[k].append(timed(e, args.steps, ini)[0])
lines.append(f"## {args.steps} steps, {args.rounds} alternating rounds: steps/s median / min / max")
base = statistics.median(rates["untempered"])
for k, v in rates.items():
    lines.append(f"{k:20s} {statistics.median(v):9.1f} {min(v):9.1f} {max(v):9.1f}   x{statistics.median(v) / base:.4f} of untempered")

# ---- 3. split-R-hat of the cold chains at equal gradient evaluations
K = C // R
lines.append(f"## split-R-hat / ESS of the log-posterior trace, warm-up {args.nwarm} (adapt), then {args.nsamp} steps: {K} cold chains of "
             f"a {C}-chain ladder run against {K} untempered chains with {R} x the steps")
e = DeviceHMC(op, SIGMA, epsilon=args.epsilon, L=L, seed=1, adapt=args.nwarm, ladder=R, beta_min=args.beta_min)
r = e.run(args.nwarm + args.nsamp, ini, store_chain=False)
d = diag.diagnose_chains(r['logpost'][::R, :, None].contiguous(), args.nwarm)
rate = r['swap_rate'].cpu().numpy().reshape(K, R)[:, :-1].mean(axis=0)
trips = pt.round_trips(r['replica'].cpu().numpy(), R)
lines.append(f"{'cold chains of the ladder':34s} R-hat {float(d['rhat'][0]):7.3f}  ESS {float(d['ess'][0]):8.1f}  mean logpost "
             f"{float(r['logpost'][::R, args.nwarm:].mean()):.1f}  swap rate per pair {np.round(rate, 2).tolist()}  round trips {int(trips.sum())}")
e = DeviceHMC(op, SIGMA, epsilon=args.epsilon, L=L, seed=1, adapt=args.nwarm)
nlong = args.nwarm + R * args.nsamp
r = e.run(nlong, ini[::R], store_chain=False)
d = diag.diagnose_chains(r['logpost'][..., None].contiguous(), args.nwarm)
lines.append(f"{'untempered, R x the steps':34s} R-hat {float(d['rhat'][0]):7.3f}  ESS {float(d['ess'][0]):8.1f}  mean logpost "
             f"{float(r['logpost'][:, args.nwarm:].mean()):.1f}")
text = "\n".join(lines) + "\n"
print(text)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(text)
