#!/usr/bin/env python3
"""Gaussian weight prior on the device engines: what the qn_prior_fold launch behind every forward / gradient call costs at the
cfg2 shape (64 chains, 3x64 tanh, N = 4096, p = 8513) on one card.  Writes profiles/prior.txt (--out).

  * qn_prior_fold alone (device events over many launches): with a float64 gradient + SSE, and the SSE alone (grad NULL)
  * steps/s of DeviceHMC (L = 3), DeviceMALA, DeviceAMCMC before its first adaptation and DeviceSGHMC (batch = 512), each with
    priorsigma = None and priorsigma = 1.0 in the same run: after a warm-up that lets the clock settle, the two variants are
    timed alternately, `--reps` windows each, and the median and the spread of the windows are reported.

The None rates are to be read against the records of the same engines without the argument (profiles/hmc_adapt.txt,
profiles/temper.txt, profiles/sgmcmc.txt, the README's device-engine table): the default path makes the same launches."""
import argparse, os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from quinn_amd import _lib
from quinn_amd.ops import MLPArch, BatchedMLP
from quinn_amd.mcmc.device_amcmc import DeviceAMCMC
from quinn_amd.mcmc.device_hmc import DeviceHMC
from quinn_amd.mcmc.device_mala import DeviceMALA
from quinn_amd.mcmc.device_sgmcmc import DeviceSGHMC

HBM_PEAK = 8.0e12


def data(N):
    rs = np.random.RandomState(0)
    x = rs.rand(N, 1) * 2 * np.pi - np.pi
    return x, 0.02 * rs.randn(N, 1) + np.sin(x)


def window(eng, n, ini):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    eng.run(n, ini, store_chain=False)
    torch.cuda.synchronize()
    return n / (time.perf_counter() - t0)


def fold_us(C, p, with_grad, reps=2000):
    """qn_prior_fold alone on [C, p] float64: microseconds per launch (device events)."""
    L, dev, f64 = _lib.lib(), "cuda", torch.float64
    W = torch.randn(C, p, dtype=f64, device=dev)
    g = torch.zeros(C, p, dtype=f64, device=dev) if with_grad else None
    sse = torch.zeros(C, dtype=f64, device=dev)
    call = lambda: _lib.check(L.qn_prior_fold(W.data_ptr(), 1e-9, 0.0, g.data_ptr() if with_grad else None, _lib.QN_F64,
                                              sse.data_ptr(), 1, C, p, None), "qn_prior_fold")
    for _ in range(200):
        call()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        call()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prior.txt"))
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    dims, N, C = (1, 64, 64, 64, 1), 4096, 64
    arch = MLPArch(dims, "tanh")
    p = arch.nparams
    x, y = data(N)
    op = BatchedMLP(arch, x, y)
    ini = np.stack([0.1 * np.random.RandomState(1000 + c).randn(p) for c in range(C)])
    lines = ["Gaussian weight prior on the device engines, %s" % torch.cuda.get_device_name(0),
             "cfg2: %d chains, p = %d, N = %d; chain not stored; priorsigma None (no launch) / 1.0 (one qn_prior_fold per forward or "
             "gradient call)" % (C, p, N),
             "windows timed alternately None, 1.0, None, ... after a warm-up run of each; median [min .. max] of %d windows" % a.reps, ""]
    for with_grad, label, nbytes in ((True, "gradient float64 + SSE", C * p * 24), (False, "SSE alone (grad NULL)   ", C * p * 8)):
        us = fold_us(C, p, with_grad)
        lines.append("qn_prior_fold alone, %s: %6.2f us per launch (device events, launches back to back); %.2f MB -> traffic "
                     "bound %.2f us at %.0f TB/s" % (label, us, nbytes / 1e6, nbytes / HBM_PEAK * 1e6, HBM_PEAK / 1e12))
    lines.append("")
    engines = [
        ("DeviceHMC  L = 3      ", lambda ps: DeviceHMC(op, 0.02, epsilon=1e-7, L=3, seed=1, priorsigma=ps), 1200),
        ("DeviceMALA            ", lambda ps: DeviceMALA(op, 0.02, epsilon=1e-7, seed=1, priorsigma=ps), 3000),
        ("DeviceAMCMC pre-adapt ", lambda ps: DeviceAMCMC(op, 0.02, t0=1 << 30, seed=1, priorsigma=ps), 8000),
        ("DeviceSGHMC batch 512 ", lambda ps: DeviceSGHMC(op, 0.02, eta=1e-9, alpha=0.1, batch=512, seed=1, priorsigma=ps), 3000),
    ]
    for label, make, n in engines:
        engs = {None: make(None), 1.0: make(1.0)}
        for e in engs.values():
            e.run(max(60, n // 4), ini, store_chain=False)                  # warm-up: code objects, buffers, clock
        rates = {None: [], 1.0: []}
        for _ in range(a.reps):
            for ps in (None, 1.0):
                rates[ps].append(window(engs[ps], n, ini))
        med = {ps: float(np.median(v)) for ps, v in rates.items()}
        for ps in (None, 1.0):
            lines.append("%s priorsigma %-4s %10.1f steps/s  [%.1f .. %.1f]" % (label, ps, med[ps], min(rates[ps]), max(rates[ps])))
        lines.append("%s with prior / without  %.3f" % (label, med[1.0] / med[None]))
        lines.append("")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
