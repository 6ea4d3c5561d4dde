#!/usr/bin/env python3
"""Hierarchical weight prior on the device HMC / MALA engines: what the per-group fold and the Gibbs round cost at the cfg2
shape (64 chains, 3x64 tanh, N = 4096, p = 8513, groups='layer': G = 4) on one card.  Writes profiles/hyper.txt (--out).

  * qn_prior_fold_g beside qn_prior_fold (device events over many launches): float64 gradient + SSE
  * qn_hyper_gibbs per round (device events; the parities flipped by the caller as in a run)
  * steps/s of DeviceHMC (L = 3) and DeviceMALA with priorsigma = 1.0 (the scalar prior: the yardstick) and with
    hyperprior = dict(a0=1, b0=1, groups='layer', every=1) in the same process: after a warm-up that lets the clock settle
    the two variants are timed alternately, `--reps` windows each, and the median and the spread of the windows are reported.

The priorsigma rates are to be read against profiles/prior.txt: the default path makes the same launches."""
import argparse, os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from quinn_amd import _lib
from quinn_amd.ops import MLPArch, BatchedMLP
from quinn_amd.mcmc import hyper as hy
from quinn_amd.mcmc.device_hmc import DeviceHMC
from quinn_amd.mcmc.device_mala import DeviceMALA

HBM_PEAK = 8.0e12
HP = dict(a0=1.0, b0=1.0, groups='layer', every=1)


def data(N):
    rs = np.random.RandomState(0)
    x = rs.rand(N, 1) * 2 * np.pi - np.pi
    return x, 0.02 * rs.randn(N, 1) + np.sin(x)


def window(eng, n, ini):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    eng.run(n, ini, store_chain=False)
    torch.cuda.synchronize()
    return n / (time.perf_counter() - t0)


def events_us(call, reps):
    for i in range(200):
        call(i)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(reps):
        call(200 + i)
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def kernel_times(C, p, seg, reps=2000):
    """(us per qn_prior_fold, per qn_prior_fold_g, per qn_hyper_gibbs) on [C, p] float64, launches back to back."""
    L, dev, f64 = _lib.lib(), "cuda", torch.float64
    G = len(seg) - 1
    W = 0.1 * torch.randn(C, p, dtype=f64, device=dev)
    g = torch.zeros(C, p, dtype=f64, device=dev)
    sse = torch.zeros(C, dtype=f64, device=dev)
    lam, c0 = hy.fold_constants_g(0.02, np.ones((C, G)), seg, HP['a0'], HP['b0'])
    lam = torch.as_tensor(np.stack([lam * 1e-6, lam * 1e-6]), device=dev)       # (tiny: the gradient stays finite over the launches)
    c0 = torch.as_tensor(np.stack([c0, c0]), device=dev)
    segt = torch.as_tensor(seg, device=dev)
    scalar = events_us(lambda i: _lib.check(L.qn_prior_fold(W.data_ptr(), 1e-9, 0.0, g.data_ptr(), _lib.QN_F64, sse.data_ptr(), 1,
                                                            C, p, None), "qn_prior_fold"), reps)
    grouped = events_us(lambda i: _lib.check(L.qn_prior_fold_g(W.data_ptr(), lam.data_ptr(), c0.data_ptr(), segt.data_ptr(), G,
                                                               g.data_ptr(), _lib.QN_F64, sse.data_ptr(), 1, C, p, None),
                                             "qn_prior_fold_g"), reps)
    nmcmc = 8
    cur_lp = torch.zeros(2, C, dtype=f64, device=dev)
    best_lp = torch.zeros(2, C, dtype=f64, device=dev)
    lps = torch.zeros(C, nmcmc + 1, dtype=f64, device=dev)
    taus = torch.ones(C, 2, G, dtype=f64, device=dev)
    step = torch.ones(2, dtype=torch.int64, device=dev)
    g.zero_()
    gibbs = events_us(lambda i: _lib.check(L.qn_hyper_gibbs(W.data_ptr(), g.data_ptr(), cur_lp.data_ptr(), best_lp.data_ptr(),
                                                            lps.data_ptr(), lam.data_ptr(), c0.data_ptr(), segt.data_ptr(),
                                                            taus.data_ptr(), step.data_ptr(), 0.02, HP['a0'], HP['b0'], G, 0, 1, C,
                                                            0, p, nmcmc, 1, i & 1, i & 1, None), "qn_hyper_gibbs"), reps)
    return scalar, grouped, gibbs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hyper.txt"))
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    dims, N, C = (1, 64, 64, 64, 1), 4096, 64
    arch = MLPArch(dims, "tanh")
    p = arch.nparams
    seg, names = hy.group_segments(arch, HP['groups'])
    G = len(names)
    x, y = data(N)
    op = BatchedMLP(arch, x, y)
    ini = np.stack([0.1 * np.random.RandomState(1000 + c).randn(p) for c in range(C)])
    parts = int(_lib.lib().qn_hmc_parts(p))
    lines = ["Hierarchical weight prior on the device HMC / MALA engines, %s" % torch.cuda.get_device_name(0),
             "cfg2: %d chains, p = %d, N = %d; chain not stored; groups = 'layer' (G = %d, bounds %s); a Gibbs round after every step"
             % (C, p, N, G, seg.tolist()),
             "priorsigma 1.0 (one qn_prior_fold per gradient call: the yardstick) / hyperprior (one qn_prior_fold_g per gradient call "
             "+ one qn_hyper_gibbs per step)",
             "windows timed alternately after a warm-up run of each; median [min .. max] of %d windows" % a.reps, ""]
    scalar, grouped, gibbs = kernel_times(C, p, seg)
    fold_bytes = C * p * 24
    gibbs_bytes = C * p * 8 * parts + C * p * 16                              # every workgroup reads the chain's row; gradient read + write
    lines += ["qn_prior_fold   alone, gradient float64 + SSE: %6.2f us per launch (device events, launches back to back); %.2f MB -> "
              "traffic bound %.2f us at %.0f TB/s" % (scalar, fold_bytes / 1e6, fold_bytes / HBM_PEAK * 1e6, HBM_PEAK / 1e12),
              "qn_prior_fold_g alone, gradient float64 + SSE: %6.2f us per launch; the same %.2f MB; per-group / scalar %.3f"
              % (grouped, fold_bytes / 1e6, grouped / scalar),
              "qn_hyper_gibbs  alone:                         %6.2f us per round; %.2f MB requested (each of a chain's %d workgroups "
              "reads the whole row, %.2f MB of it unique; gradient read + written) -> traffic bound %.2f us at %.0f TB/s"
              % (gibbs, gibbs_bytes / 1e6, parts, C * p * 8 / 1e6, gibbs_bytes / HBM_PEAK * 1e6, HBM_PEAK / 1e12), ""]
    engines = [
        ("DeviceHMC  L = 3 ", lambda kw: DeviceHMC(op, 0.02, epsilon=1e-7, L=3, seed=1, **kw), 1200),
        ("DeviceMALA       ", lambda kw: DeviceMALA(op, 0.02, epsilon=1e-7, seed=1, **kw), 3000),
    ]
    for label, make, n in engines:
        engs = {'priorsigma 1.0': make(dict(priorsigma=1.0)), 'hyperprior    ': make(dict(hyperprior=HP))}
        for e in engs.values():
            e.run(max(60, n // 4), ini, store_chain=False)                  # warm-up: code objects, buffers, clock
        rates = {k: [] for k in engs}
        for _ in range(a.reps):
            for k in engs:
                rates[k].append(window(engs[k], n, ini))
        med = {k: float(np.median(v)) for k, v in rates.items()}
        for k in engs:
            lines.append("%s %s %10.1f steps/s  [%.1f .. %.1f]" % (label, k, med[k], min(rates[k]), max(rates[k])))
        lines.append("%s hyperprior / priorsigma  %.3f" % (label, med['hyperprior    '] / med['priorsigma 1.0']))
        lines.append("")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
