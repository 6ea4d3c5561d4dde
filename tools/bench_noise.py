#!/usr/bin/env python3
"""Sampled noise level on the device HMC / MALA engines: what the fused fold and the extra Gibbs round cost at the cfg2 shape
(64 chains, 3x64 tanh, N = 4096, p = 8513, groups='layer': G = 4) on one card.  Writes profiles/noise.txt (--out).

  * qn_noise_fold beside qn_prior_fold_g (G = 4), float64 gradient + SSE: device events over many launches, the two kernels
    timed alternately in one process, `--reps` windows each
  * qn_noise_gibbs per round (device events; a self-consistent state, the parities flipped by the caller as in a run)
  * steps/s of DeviceHMC (L = 3) and DeviceMALA with hyperprior alone (the parent's path: the yardstick) and with
    hyperprior + noiseprior in the same process: after a warm-up run of each the two variants are timed alternately, `--reps`
    windows each, and the median and the spread of the windows are reported.

The hyperprior rates are to be read against profiles/hyper.txt: that path makes the same launches as before."""
import argparse, os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from quinn_amd import _lib
from quinn_amd.ops import MLPArch, BatchedMLP
from quinn_amd.mcmc import hyper as hy
from quinn_amd.mcmc import noise as nz
from quinn_amd.mcmc.device_hmc import DeviceHMC
from quinn_amd.mcmc.device_mala import DeviceMALA

HBM_PEAK = 8.0e12
HP = dict(a0=1.0, b0=1.0, groups='layer', every=1)
NP = dict(a0=2.0, b0=1e-3, every=1)
SIGMA = 0.02


def data(N):
    rs = np.random.RandomState(0)
    x = rs.rand(N, 1) * 2 * np.pi - np.pi
    return x, SIGMA * rs.randn(N, 1) + np.sin(x)


def window(eng, n, ini):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    eng.run(n, ini, store_chain=False)
    torch.cuda.synchronize()
    return n / (time.perf_counter() - t0)


def events_us(call, reps, warm=200):
    for i in range(warm):
        call(i)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(reps):
        call(warm + i)
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def kernel_times(C, p, N, seg, windows, reps=2000):
    """([us per qn_prior_fold_g], [us per qn_noise_fold], [us per qn_noise_gibbs]) on [C, p] float64, launches back to back."""
    L, dev, f64 = _lib.lib(), "cuda", torch.float64
    G = len(seg) - 1
    rs = np.random.RandomState(0)
    W = 0.1 * rs.randn(C, p)
    lam, c0 = hy.fold_constants_g(SIGMA, np.ones((C, G)), seg, HP['a0'], HP['b0'])
    lam = lam * 1e-6                                                          # (tiny: the gradient stays finite over the launches)
    kappa, d0 = nz.fold_constants_n(SIGMA, np.full(C, SIGMA * SIGMA), N, N, NP['a0'], NP['b0'])
    h, lik_const = nz.lik_constants(SIGMA, N)
    cur_lp = -(h * nz.fold_n(W, kappa, d0, lam, c0, seg, sse=np.full(C, N * SIGMA * SIGMA))[1] + lik_const)
    Wt, g, sse = torch.as_tensor(W, device=dev), torch.zeros(C, p, dtype=f64, device=dev), torch.zeros(C, dtype=f64, device=dev)
    lamt, c0t, segt = torch.as_tensor(lam, device=dev), torch.as_tensor(c0, device=dev), torch.as_tensor(seg, device=dev)
    one, zero = torch.ones(C, dtype=f64, device=dev), torch.zeros(C, dtype=f64, device=dev)

    def fold_g(i):
        _lib.check(L.qn_prior_fold_g(Wt.data_ptr(), lamt.data_ptr(), c0t.data_ptr(), segt.data_ptr(), G, g.data_ptr(), _lib.QN_F64,
                                     sse.data_ptr(), 1, C, p, None), "qn_prior_fold_g")

    def fold_n(i):
        _lib.check(L.qn_noise_fold(Wt.data_ptr(), one.data_ptr(), zero.data_ptr(), lamt.data_ptr(), c0t.data_ptr(), segt.data_ptr(),
                                   G, g.data_ptr(), _lib.QN_F64, sse.data_ptr(), 1, C, p, None), "qn_noise_fold")
    tg, tn = [], []
    for _ in range(windows):
        tg.append(events_us(fold_g, reps))
        tn.append(events_us(fold_n, reps))
    nmcmc = 8
    clp = torch.as_tensor(np.stack([cur_lp, cur_lp]), device=dev)
    best_lp = torch.zeros(2, C, dtype=f64, device=dev)
    lps = torch.zeros(C, nmcmc + 1, dtype=f64, device=dev)
    kap, d0t = torch.as_tensor(np.stack([kappa, kappa]), device=dev), torch.as_tensor(np.stack([d0, d0]), device=dev)
    sig = torch.ones(C, 2, dtype=f64, device=dev)
    step = torch.ones(2, dtype=torch.int64, device=dev)
    g.zero_()

    def gibbs(i):
        _lib.check(L.qn_noise_gibbs(Wt.data_ptr(), g.data_ptr(), clp.data_ptr(), best_lp.data_ptr(), lps.data_ptr(), kap.data_ptr(),
                                    d0t.data_ptr(), lamt.data_ptr(), c0t.data_ptr(), segt.data_ptr(), sig.data_ptr(),
                                    None, step.data_ptr(), SIGMA, NP['a0'], NP['b0'], N, N, G, 0, 1, C, 0, p, nmcmc, 1, i & 1, i & 1, None),
                   "qn_noise_gibbs")
    tr = [events_us(gibbs, reps) for _ in range(windows)]
    moved = float((sig[:, 1] != 1.0).double().mean())                        # (the share of chains whose last round drew)
    return tg, tn, tr, moved


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "noise.txt"))
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
    lines = ["Sampled noise level on the device HMC / MALA engines, %s" % torch.cuda.get_device_name(0),
             "cfg2: %d chains, p = %d, N = %d; chain not stored; groups = 'layer' (G = %d); a Gibbs round of each kind after every step"
             % (C, p, N, G),
             "hyperprior (one qn_prior_fold_g per gradient call + one qn_hyper_gibbs per step: the yardstick) / hyperprior + noiseprior "
             "(one qn_noise_fold per gradient call + one qn_hyper_gibbs + one qn_noise_gibbs per step)",
             "windows timed alternately after a warm-up; median [min .. max] of %d windows" % a.reps, ""]
    tg, tn, tr, moved = kernel_times(C, p, N, seg, a.reps)
    fold_bytes = C * p * 24
    gibbs_bytes = C * p * 8 * parts + C * p * 24
    med = lambda v: float(np.median(v))
    lines += ["qn_prior_fold_g alone, gradient float64 + SSE: %6.2f us per launch [%.2f .. %.2f] (device events, launches back to "
              "back); %.2f MB -> traffic bound %.2f us at %.0f TB/s"
              % (med(tg), min(tg), max(tg), fold_bytes / 1e6, fold_bytes / HBM_PEAK * 1e6, HBM_PEAK / 1e12),
              "qn_noise_fold   alone, gradient float64 + SSE: %6.2f us per launch [%.2f .. %.2f]; the same %.2f MB; fused / per-group %.3f"
              % (med(tn), min(tn), max(tn), fold_bytes / 1e6, med(tn) / med(tg)),
              "qn_noise_gibbs  alone:                         %6.2f us per round [%.2f .. %.2f]; %.2f MB requested (each of a chain's "
              "%d workgroups reads the whole row for the group sums; weights + gradient read, gradient written) -> traffic bound "
              "%.2f us at %.0f TB/s; %.0f %% of the chains drew in the last round"
              % (med(tr), min(tr), max(tr), gibbs_bytes / 1e6, parts, gibbs_bytes / HBM_PEAK * 1e6, HBM_PEAK / 1e12, 100 * moved), ""]
    engines = [
        ("DeviceHMC  L = 3 ", lambda kw: DeviceHMC(op, SIGMA, epsilon=1e-7, L=3, seed=1, **kw), 1200),
        ("DeviceMALA       ", lambda kw: DeviceMALA(op, SIGMA, epsilon=1e-7, seed=1, **kw), 3000),
    ]
    for label, make, n in engines:
        engs = {'hyperprior             ': make(dict(hyperprior=HP)),
                'hyperprior + noiseprior': make(dict(hyperprior=HP, noiseprior=NP))}
        for e in engs.values():
            e.run(max(60, n // 4), ini, store_chain=False)                  # warm-up: code objects, buffers, clock
        rates = {k: [] for k in engs}
        for _ in range(a.reps):
            for k in engs:
                rates[k].append(window(engs[k], n, ini))
        m = {k: float(np.median(v)) for k, v in rates.items()}
        for k in engs:
            lines.append("%s %s %10.1f steps/s  [%.1f .. %.1f]" % (label, k, m[k], min(rates[k]), max(rates[k])))
        lines.append("%s with noiseprior / without  %.3f" % (label, m['hyperprior + noiseprior'] / m['hyperprior             ']))
        lines.append("")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
