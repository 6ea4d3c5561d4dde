#!/usr/bin/env python3
"""Device elliptical slice sampling at the cfg2 shape (64 chains, 3x64 tanh, N = 4096), priorsigma = 1.0, one MI355X: stored
steps/s, forward evaluations per step (mean / max of `nev`), truncated steps, the share of launches in which fewer than all
chains were live, and one qn_ess_iter launch in both branches (device events) beside its byte count; in the same run `DeviceHMC`
(L = 3), `DeviceMALA` and `DeviceAMCMC` with the same priorsigma, and for each sampler split-R-hat and batch-means ESS of the
log-posterior trace (second half of the run) per second -- the ESS only where the chains agree (R-hat <= 1.1).  Writes
profiles/ess.txt (--out).  The gradient samplers' step size is the one of tools/bench_prior.py; no tuning is attempted here, and
no ratio is claimed."""
import argparse, os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from quinn_amd import _lib
from quinn_amd.ops import MLPArch, BatchedMLP
from quinn_amd.mcmc import diagnostics as diag
from quinn_amd.mcmc.device_amcmc import DeviceAMCMC
from quinn_amd.mcmc.device_ess import DeviceESS
from quinn_amd.mcmc.device_hmc import DeviceHMC
from quinn_amd.mcmc.device_mala import DeviceMALA

HBM_PEAK = 8.0e12


def data(N):
    rs = np.random.RandomState(0)
    x = rs.rand(N, 1) * 2 * np.pi - np.pi
    return x, 0.02 * rs.randn(N, 1) + np.sin(x)


def timed(eng, n, ini, warm):
    eng.run(warm, ini)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    res = eng.run(n, ini)
    torch.cuda.synchronize()
    return res, time.perf_counter() - t0


def trace_stats(res, n, dt, dev):
    """'R-hat r, min ESS e, e / dt ESS/s' of the log-posterior trace; the ESS of chains that do not agree (R-hat > 1.1) means
    nothing and is not printed."""
    d = diag.diagnose_chains(res['logpost'][..., None], n // 2, device=dev)
    rhat, ess_min = float(np.max(d['rhat'])), float(np.min(d['ess']))
    if not rhat <= 1.1:
        return "R-hat %.3f, ESS n/a (R-hat > 1.1: the chains have not converged)" % rhat
    return "R-hat %.3f, min ESS %.1f, %.1f ESS/s" % (rhat, ess_min, ess_min / dt)


def iter_kernel_us(C, p, accept, reps=300):
    """qn_ess_iter alone on [C, p] float64, no chain stored, every chain in the same branch: (us per launch, bytes per launch)."""
    L, dev, f64 = _lib.lib(), "cuda", torch.float64
    nmcmc = reps + 64
    cur = torch.randn(C, p, dtype=f64, device=dev)
    nu, prop, best = torch.empty_like(cur), torch.empty_like(cur), cur.clone()
    sse0, lp0 = torch.ones(C, dtype=f64, device=dev), torch.zeros(C, dtype=f64, device=dev)
    nwg = int(L.qn_hmc_parts(p))
    sq, es = torch.zeros(2, C, nwg, dtype=f64, device=dev), torch.zeros(2, C, 6, dtype=f64, device=dev)
    ei = torch.zeros(2, C, 4, dtype=torch.int64, device=dev)
    best_lp = torch.full((2, C), float('inf'), dtype=f64, device=dev)            # never better: no best row is written
    lps, nev = torch.zeros(C, nmcmc + 1, dtype=f64, device=dev), torch.zeros(C, nmcmc + 1, dtype=torch.int32, device=dev)
    _lib.check(L.qn_ess_begin(cur.data_ptr(), sse0.data_ptr(), lp0.data_ptr(), 0.02, 1.0, C, 0, p, 1, nu.data_ptr(), prop.data_ptr(),
                              None, _lib.QN_F64, sq.data_ptr(), es.data_ptr(), ei.data_ptr(), None), "qn_ess_begin")
    sse = torch.full((C, 1), 0.0 if accept else 1e300, dtype=f64, device=dev)   # gs sse = 0 > logy always; -1e303 never
    call = lambda par: _lib.check(L.qn_ess_iter(sse.data_ptr(), 1, 0.02, 1.0, 4096, 1 << 30, C, 0, p, nmcmc, 1, cur.data_ptr(),
                                                nu.data_ptr(), prop.data_ptr(), None, _lib.QN_F64, best.data_ptr(), best_lp.data_ptr(),
                                                None, lps.data_ptr(), nev.data_ptr(), sq.data_ptr(), es.data_ptr(), ei.data_ptr(),
                                                par, None), "qn_ess_iter")
    for i in range(20):
        call(i & 1)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(reps):
        call(i & 1)
    e1.record(); torch.cuda.synchronize()
    assert int(ei[0, 0, 0 if accept else 1]) == 20 + reps                         # every launch took the branch that is timed
    return e0.elapsed_time(e1) * 1e3 / reps, C * p * 8 * (4 if accept else 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ess.txt"))
    ap.add_argument("--steps", type=int, default=2000)
    a = ap.parse_args()
    dev, n, ps, sigma = "cuda", a.steps, 1.0, 0.02
    arch, N, C = MLPArch((1, 64, 64, 64, 1), "tanh"), 4096, 64
    x, y = data(N)
    op = BatchedMLP(arch, x, y)
    ini = np.stack([0.1 * np.random.RandomState(1000 + c).randn(arch.nparams) for c in range(C)])
    lines = ["device elliptical slice sampling, cfg2: %d chains, p = %d, N = %d, sigma = %g, priorsigma = %g, %d stored steps, chain "
             "stored, %s (%s)" % (C, arch.nparams, N, sigma, ps, n, torch.cuda.get_device_name(0),
                                  getattr(torch.cuda.get_device_properties(0), "gcnArchName", "arch unknown")),
             "R-hat / ESS: split-R-hat and batch-means ESS of the log-posterior trace over the %d chains, rows %d .. %d" % (C, n // 2, n), ""]
    eng = DeviceESS(op, sigma, priorsigma=ps, seed=1)
    res, dt = timed(eng, n, ini, max(8, n // 10))
    nev = res['nev'][:, 1:].double()
    nevals = res['nevals'].cpu().numpy()
    enq, needed = eng.last_iters
    lines += ["DeviceESS (max_shrink 32, block 32)  %10.1f stored steps/s per chain (%.1f forward evaluations/s over all chains)"
              % (n / dt, float(nevals.sum()) / dt),
              "  forward evaluations per step: mean %.3f, max %d; truncated steps %d" % (float(nev.mean()), int(nev.max()), int(res['ntrunc'].sum())),
              "  iterations: slowest chain %d, fastest chain %d; launches with fewer than all chains live: %.2f %% of the %d needed; "
              "%d enqueued (whole blocks, one block late)" % (nevals.max(), nevals.min(), 100.0 * (nevals.max() - nevals.min()) / nevals.max(),
                                                              nevals.max(), enq),
              "  log-posterior trace: " + trace_stats(res, n, dt, dev)]
    for accept, label in ((True, "accept (read prop; write cur, nu, prop)"), (False, "shrink (read cur, nu; write prop)")):
        us, nbytes = iter_kernel_us(C, arch.nparams, accept)
        lines.append("  qn_ess_iter alone, %s: %.2f us per launch, %.2f MB -> %.2f TB/s; traffic bound %.2f us at %.1f TB/s (peak)"
                     % (label, us, nbytes / 1e6, nbytes / us / 1e6, nbytes / HBM_PEAK * 1e6, HBM_PEAK / 1e12))
    lines.append("")
    for name, mk in (("DeviceHMC (L = 3, epsilon 1e-7)", lambda: DeviceHMC(op, sigma, epsilon=1e-7, L=3, seed=1, priorsigma=ps)),
                     ("DeviceMALA (epsilon 1e-7)", lambda: DeviceMALA(op, sigma, epsilon=1e-7, seed=1, priorsigma=ps)),
                     ("DeviceAMCMC (gamma 0.1)", lambda: DeviceAMCMC(op, sigma, seed=1, priorsigma=ps))):
        res, dt = timed(mk(), n, ini, max(8, n // 10))
        lines.append("%-36s %10.1f steps/s per chain, acceptance %.3f; log-posterior trace: %s"
                     % (name, n / dt, float(res['accrate'].mean()), trace_stats(res, n, dt, dev)))
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
