#!/usr/bin/env python3
"""Device NUTS at the cfg2 shape (64 chains, 3x64 tanh, N = 4096), one MI355X.  `DeviceHMC` (L = 3) and `DeviceNUTS` each run a
warm-up of their own (--warm steps) and --steps further steps from the same starts; a second `DeviceNUTS` run takes the step sizes
and the diagonal mass of that `DeviceHMC` run, from its last states.  Recorded per run: gradient evaluations/s, and for NUTS depth
and leapfrogs per step, divergent steps, steps stopped by max_depth, the share of launches in which fewer than all chains were
live; one gradient launch (qn_mlp_sse_fwdbwd) alone and one qn_nuts_iter alone (device events) for a leaf inside a subtree and
for a merge that doubles, each beside its byte count and its traffic bound at 8 TB/s; and split-R-hat and batch-means ESS of the
log-posterior trace (the last half of the steps after the warm-up) per second -- the ESS only where the chains agree (R-hat <=
1.1).  Writes profiles/nuts.txt (--out).  No ratio is claimed."""
import argparse, os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from quinn_amd import _lib
from quinn_amd.ops import MLPArch, BatchedMLP
from quinn_amd.mcmc.device_hmc import DeviceHMC
from quinn_amd.mcmc.device_nuts import DeviceNUTS
from bench_ess import HBM_PEAK, data, trace_stats

VEC = DeviceNUTS._VEC


def iter_kernel_us(C, p, merge, reps=200):
    """qn_nuts_iter alone on [C, p] float64 with a scale, no chain stored, every chain in the same branch and the state rewound
    before every launch (a 20-number copy per chain, outside the timed events' kernels but between them: subtracted as measured
    alone): (us per launch, bytes per launch).  merge = False: leaf 2 of 8 (even: stores a checkpoint); True: leaf 1 of 2
    completes doubling 1, is merged and the next subtree starts."""
    L, dev, f64 = _lib.lib(), "cuda", torch.float64
    D = 10
    s = {k: torch.rand(C, p, dtype=f64, device=dev) + 0.5 for k in VEC[:14]}      # momenta all point the same way: no U-turn
    s['ck_u'], s['ck_rho'] = torch.rand(C, D, p, dtype=f64, device=dev) + 0.5, 0.1 * torch.rand(C, D, p, dtype=f64, device=dev)
    scale, best = torch.ones(C, p, dtype=f64, device=dev), torch.zeros(C, p, dtype=f64, device=dev)
    nwg = int(L.qn_hmc_parts(p))
    es, ei = torch.zeros(2, C, 12, dtype=f64, device=dev), torch.zeros(2, C, 8, dtype=torch.int64, device=dev)
    es[:, :, 0], es[:, :, 4], es[:, :, 5] = 1e-6, 0.5 * 1.1 * p, (50.0 if not merge else -50.0)   # eps, H0 ~ |u|^2 / 2, logW
    ei[:, :, 1:5] = torch.as_tensor([1, 1, 1, 1] if merge else [3, 2, 1, 2], device=dev)
    es0, ei0 = es.clone(), ei.clone()
    best_lp = torch.full((2, C), float('inf'), dtype=f64, device=dev)
    rows = [torch.zeros(C, 3, dtype=t, device=dev) for t in (f64, f64, torch.int32, torch.int32)]
    dots, zz = torch.zeros(C, nwg, 27, dtype=f64, device=dev), torch.zeros(2, C, nwg, dtype=f64, device=dev)
    sse, grad = torch.zeros(C, dtype=f64, device=dev), 1e-3 * torch.randn(C, p, dtype=f64, device=dev)

    def call():
        es.copy_(es0); ei.copy_(ei0)
        _lib.check(L.qn_nuts_iter(sse.data_ptr(), grad.data_ptr(), scale.data_ptr(), 0.02, 4096, D, 0, 0.8, C, 0, p, 2, 1,
                                  *(s[k].data_ptr() for k in VEC), best.data_ptr(), best_lp.data_ptr(), None, rows[0].data_ptr(),
                                  rows[1].data_ptr(), rows[2].data_ptr(), rows[3].data_ptr(), dots.data_ptr(), zz.data_ptr(),
                                  es.data_ptr(), ei.data_ptr(), 0, None), "qn_nuts_iter")

    def timed(fn):
        for _ in range(20):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / reps

    rewind = timed(lambda: (es.copy_(es0), ei.copy_(ei0)))
    us = timed(call) - rewind
    want = (0, 2, 0) if merge else (0, 3, 3)                         # (t, d, i) after the launch: the branch that is timed
    assert tuple(int(v) for v in ei[1, 0, :3]) == want, ei[1, 0]
    # vectors moved, 8 B per element each, the scale read in both kernels: leaf -- reduce u g rho_sub s -> u rho_sub ck_u ck_rho,
    # decide q u g s -> q u sub_q sub_g (the leaf is taken as the subtree's proposal here); merge -- reduce u g rho_sub s ck_u ck_rho
    # rho edge -> u rho_sub, decide q u g sub_q sub_g rho rho_sub s other edge (3) -> cur gcur rho edge (3) q u
    return us, C * p * 8 * (23 if merge else 16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nuts.txt"))
    ap.add_argument("--steps", type=int, default=600)
    ap.add_argument("--warm", type=int, default=300)
    ap.add_argument("--max-depth", dest="max_depth", type=int, default=8)
    a = ap.parse_args()
    dev, n, sigma = "cuda", a.steps, 0.02
    arch, N, C = MLPArch((1, 64, 64, 64, 1), "tanh"), 4096, 64
    x, y = data(N)
    op = BatchedMLP(arch, x, y)
    p = arch.nparams
    ini = np.stack([0.1 * np.random.RandomState(1000 + c).randn(p) for c in range(C)])
    W, D = a.warm, a.max_depth
    lines = ["device NUTS, cfg2: %d chains, p = %d, N = %d, sigma = %g, no prior, %d warm-up + %d stored steps, chain stored, %s (%s)"
             % (C, p, N, sigma, W, n, torch.cuda.get_device_name(0), getattr(torch.cuda.get_device_properties(0), "gcnArchName", "arch unknown")),
             "R-hat / ESS: split-R-hat and batch-means ESS of the log-posterior trace over the %d chains, the last %d rows" % (C, n - n // 2), ""]

    def timed(eng, steps, start):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        res = eng.run(steps, start)
        torch.cuda.synchronize()
        return res, time.perf_counter() - t0

    def trace(res, steps, dt):
        return trace_stats({'logpost': res['logpost'][:, steps - n:].contiguous()}, n, dt, dev)

    def nuts_lines(name, eng, res, steps, dt):
        ngrad, post = res['ngrad'].cpu().numpy(), slice(steps - n + 1, None)
        return ["%s  %10.1f stored steps/s per chain, %.1f gradient evaluations/s over all chains" % (name, steps / dt, float(ngrad.sum()) / dt),
                "  the last %d steps: depth mean %.3f, max %d; leapfrogs per step mean %.2f; acceptance statistic %.3f; step sizes %.3g .. %.3g"
                % (n, float(res['depth'][:, post].double().mean()), int(res['depth'][:, post].max()), float(res['nleap'][:, post].double().mean()),
                   float(res['alphas'][:, post].mean()), float(res['epsilon'].min()), float(res['epsilon'].max())),
                "  whole run: divergent steps %d, stopped by max_depth %d, of %d" % (int(res['ndiv'].sum()), int(res['ntreedepth'].sum()), steps * C),
                "  iterations: slowest chain %d, fastest chain %d; launches with fewer than all chains live: %.2f %% of the %d needed; %d "
                "enqueued (whole blocks, one block late)" % (ngrad.max(), ngrad.min(), 100.0 * (ngrad.max() - ngrad.min()) / ngrad.max(),
                                                             ngrad.max(), eng.last_iters[0]),
                "  log-posterior trace: " + trace(res, steps, dt)]

    # ---- every sampler with a warm-up of its own, from the same starts
    rh, dth = timed(DeviceHMC(op, sigma, epsilon=1e-7, L=3, seed=1, adapt=W), W + n, ini)
    lines.append("DeviceHMC (L = 3, adapt = %d from epsilon 1e-7: step sizes %.3g .. %.3g, mass windows %s)  %10.1f steps/s per chain = %.1f "
                 "gradient evaluations/s over all chains, acceptance %.3f; log-posterior trace: %s"
                 % (W, float(rh['epsilon'].min()), float(rh['epsilon'].max()), "yes" if rh['mass_scale'] is not None else "no",
                    (W + n) / dth, 3.0 * (W + n) * C / dth, float(rh['accrate'].mean()), trace(rh, W + n, dth)))
    eng = DeviceNUTS(op, sigma, epsilon=1e-3, adapt=W, max_depth=D, seed=2)
    r, dt = timed(eng, W + n, ini)
    lines += nuts_lines("DeviceNUTS (max_depth %d, block 32, adapt = %d from epsilon 1e-3, unit mass)" % (D, W), eng, r, W + n, dt)
    # ---- the hand-over: step sizes and mass of that HMC run, from where it ended
    eng = DeviceNUTS(op, sigma, epsilon=rh['epsilon'], mass_scale=rh['mass_scale'], max_depth=D, seed=3)
    r, dt = timed(eng, n, rh['chain'][:, -1].cpu().numpy())
    lines += nuts_lines("DeviceNUTS (max_depth %d, epsilon and mass_scale of the DeviceHMC run above, from its last states)" % D, eng, r, n, dt)
    # ---- the gradient launch alone, and qn_nuts_iter alone in two branches
    Wt = torch.as_tensor(ini, device=dev)
    out = (torch.empty(C, dtype=torch.float64, device=dev), torch.empty(C, p, dtype=torch.float64, device=dev))
    for _ in range(20):
        op.sse_grad(Wt, out=out)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(200):
        op.sse_grad(Wt, out=out)
    e1.record(); torch.cuda.synchronize()
    lines += ["", "  gradient launch alone (qn_mlp_sse_fwdbwd, %d chains): %.2f us" % (C, e0.elapsed_time(e1) * 1e3 / 200)]
    for merge, label in ((False, "leaf inside a subtree (even: stores a checkpoint)"), (True, "last leaf of doubling 1: merge, double, next subtree started")):
        us, nbytes = iter_kernel_us(C, p, merge)
        lines.append("  qn_nuts_iter alone (two launches), %s: %.2f us, %.2f MB -> %.2f TB/s; traffic bound %.2f us at %.1f TB/s (peak)"
                     % (label, us, nbytes / 1e6, nbytes / us / 1e6, nbytes / HBM_PEAK * 1e6, HBM_PEAK / 1e12))
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
