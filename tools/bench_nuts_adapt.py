#!/usr/bin/env python3
"""NUTS warm-up with and without mass windows at the cfg2 shape (64 chains, 3x64 tanh, N = 4096), one MI355X: the cfg2 run of
tools/bench_nuts.py (`DeviceNUTS`, --warm warm-up steps from epsilon 1e-3 and --steps further steps, max_depth 8) with
adapt_mass=False and adapt_mass=True, alternately in one process (--rounds of the pair, from the same starts).  Recorded per run:
leapfrogs per step after the warm-up, steps stopped by max_depth, divergent steps, the settled step sizes, the range of the
scales, gradient evaluations/s and split-R-hat of the log-posterior trace (ESS per second only where the chains agree, R-hat <=
1.1); qn_nuts_adapt alone (device events) at a collecting step and at a window end, each beside its byte count, its traffic
bound at 8 TB/s, and qn_nuts_iter alone; and the numpy contract's ill-scaled Gaussian (tests/test_nuts_adapt_contract.py), run
on the CPU.  Writes profiles/nuts_adapt.txt (--out).  No ratio is claimed."""
import argparse, os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from quinn_amd import _lib
from quinn_amd.ops import MLPArch, BatchedMLP
from quinn_amd.mcmc import nuts, nuts_adapt as na
from quinn_amd.mcmc.device_nuts import DeviceNUTS
from bench_ess import HBM_PEAK, data, trace_stats
from bench_nuts import iter_kernel_us


def adapt_kernel_us(C, p, k, adapt=300, nmcmc=900, reps=200):
    """qn_nuts_adapt alone on [C, p] float64 with every chain having just ended warm-up step k: (us per launch, bytes per launch).
    Nothing has to be rewound: the counters are not written, and ws alternates harmlessly (the same slot is read every time)."""
    L, dev, f64 = _lib.lib(), "cuda", torch.float64
    v = {n: torch.rand(C, p, dtype=f64, device=dev) + 0.5 for n in ('cur', 'ql', 'ul', 'gl', 'q', 'u', 'mean', 'm2', 'scale')}
    alphas = torch.full((C, nmcmc + 1), 0.8, dtype=f64, device=dev)
    es, ei = torch.zeros(2, C, 12, dtype=f64, device=dev), torch.zeros(2, C, 8, dtype=torch.int64, device=dev)
    ei[0, :, 0], ei[1, :, 0], ei[1, :, 3] = k - 1, k, 1
    ws = torch.zeros(2, C, 4, dtype=f64, device=dev)
    ws[0, :, 0] = np.log(10 * 1e-3)
    plan = torch.as_tensor(na.plan_table(adapt), device=dev)
    row = plan[k - 1].cpu().numpy()

    def call():
        _lib.check(L.qn_nuts_adapt(v['cur'].data_ptr(), alphas.data_ptr(), nmcmc, adapt, 0.8, plan.data_ptr(), es.data_ptr(),
                                   ei.data_ptr(), 0, C, p, 0.02, v['ql'].data_ptr(), v['ul'].data_ptr(), v['gl'].data_ptr(),
                                   v['q'].data_ptr(), v['u'].data_ptr(), ws.data_ptr(), v['mean'].data_ptr(), v['m2'].data_ptr(),
                                   v['scale'].data_ptr(), None), "qn_nuts_adapt")

    for _ in range(20):
        call()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        call()
    e1.record(); torch.cuda.synchronize()
    nvec = 6 + (5 if row[2] & na.PLAN_COLLECT else 0) + (1 if row[2] & na.PLAN_FINISH else 0)
    return e0.elapsed_time(e1) * 1e3 / reps, C * p * 8 * nvec


def contract_lines():
    sd = np.array([1.0, 0.01] * 4)
    target = lambda q: (-0.5 * float(np.sum((q / sd) ** 2)), -q / sd ** 2)
    q0 = sd * np.array([0.5, -1.0, 1.5, 0.3, -0.7, 1.1, -0.2, 0.8])
    unit = nuts.nuts_run(target, q0, 0.01, 500, max_depth=8, adapt=300, seed=3)
    wind = na.nuts_run_adapted(target, q0, 0.01, 500, max_depth=8, adapt=300, seed=3)
    return ["numpy contract (CPU), Gaussian with p = 8 and standard deviations alternating 1 and 0.01, adapt = 300 + 200 steps, max_depth 8, "
            "one chain:", "  mean leapfrogs per step after the warm-up: unit mass %.1f (step size %.3g), with windows %.1f (step size %.3g)"
            % (unit['nleap'][301:].mean(), unit['epsilon'], wind['nleap'][301:].mean(), wind['epsilon'])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nuts_adapt.txt"))
    ap.add_argument("--steps", type=int, default=600)
    ap.add_argument("--warm", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=1)
    ap.add_argument("--max-depth", dest="max_depth", type=int, default=8)
    a = ap.parse_args()
    dev, n, sigma, W, D = "cuda", a.steps, 0.02, a.warm, a.max_depth
    arch, N, C = MLPArch((1, 64, 64, 64, 1), "tanh"), 4096, 64
    x, y = data(N)
    op = BatchedMLP(arch, x, y)
    p = arch.nparams
    ini = np.stack([0.1 * np.random.RandomState(1000 + c).randn(p) for c in range(C)])
    lines = ["NUTS warm-up with and without mass windows, cfg2: %d chains, p = %d, N = %d, sigma = %g, no prior, %d warm-up + %d stored "
             "steps from epsilon 1e-3, max_depth %d, chain stored, %s (%s)" % (C, p, N, sigma, W, n, D, torch.cuda.get_device_name(0),
             getattr(torch.cuda.get_device_properties(0), "gcnArchName", "arch unknown")),
             "R-hat / ESS: split-R-hat and batch-means ESS of the log-posterior trace over the %d chains, the last %d rows" % (C, n - n // 2), ""]
    for rnd in range(a.rounds):
        for mass in (False, True):
            eng = DeviceNUTS(op, sigma, epsilon=1e-3, adapt=W, max_depth=D, seed=2, adapt_mass=mass)
            torch.cuda.synchronize(); t0 = time.perf_counter()
            r = eng.run(W + n, ini)
            torch.cuda.synchronize(); dt = time.perf_counter() - t0
            post, ngrad = slice(W + 1, None), r['ngrad'].cpu().numpy()
            lines += ["round %d, adapt_mass=%s  %.1f stored steps/s per chain, %.1f gradient evaluations/s over all chains"
                      % (rnd, mass, (W + n) / dt, float(ngrad.sum()) / dt),
                      "  after the warm-up: leapfrogs per step mean %.2f, depth mean %.3f; acceptance statistic %.3f; step sizes %.3g .. %.3g%s"
                      % (float(r['nleap'][:, post].double().mean()), float(r['depth'][:, post].double().mean()),
                         float(r['alphas'][:, post].mean()), float(r['epsilon'].min()), float(r['epsilon'].max()),
                         "; scales %.3g .. %.3g" % (float(r['mass_scale'].min()), float(r['mass_scale'].max())) if mass else ""),
                      "  whole run: stopped by max_depth %d, divergent steps %d, of %d; iterations: slowest chain %d, %d enqueued"
                      % (int(r['ntreedepth'].sum()), int(r['ndiv'].sum()), (W + n) * C, ngrad.max(), eng.last_iters[0]),
                      "  log-posterior trace: " + trace_stats({'logpost': r['logpost'][:, W:].contiguous()}, n, dt, dev)]
    lines.append("")
    for k, label in ((120, "a collecting step"), (150, "a window end")):
        us, nbytes = adapt_kernel_us(C, p, k)
        lines.append("  qn_nuts_adapt alone, every chain at %s: %.2f us, %.2f MB -> %.2f TB/s; traffic bound %.2f us at %.1f TB/s (peak)"
                     % (label, us, nbytes / 1e6, nbytes / us / 1e6, nbytes / HBM_PEAK * 1e6, HBM_PEAK / 1e12))
    us, nbytes = iter_kernel_us(C, p, False)
    lines.append("  qn_nuts_iter alone (two launches), leaf inside a subtree: %.2f us, %.2f MB" % (us, nbytes / 1e6))
    lines += [""] + contract_lines()
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
