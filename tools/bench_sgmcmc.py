#!/usr/bin/env python3
"""Device SGHMC: inner steps/s at the cfg2 (64 chains, 3x64, N=4096) and cfg5 (256 chains, 4x256, N=32768) shapes for
batch = 512, 2048 and all rows, beside `DeviceMALA` (HMC with L = 1: one full-data gradient per step) on the same card; and
the time of the step kernel alone (qn_sg_step, device events) against its HBM traffic.  Writes profiles/sgmcmc.txt (--out).

profiles/hbm_traffic.json records bytes per launch of the gradient kernels, not a rate; the traffic bound uses the rates
DESIGN section 3 works with: the 8 TB/s HBM peak and 4.3 TB/s, the best streaming rate this project measured (k_hist_block16)."""
import argparse, os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from quinn_amd import _lib
from quinn_amd.ops import MLPArch, BatchedMLP
from quinn_amd.mcmc.device_mala import DeviceMALA
from quinn_amd.mcmc.device_sgmcmc import DeviceSGHMC

HBM_PEAK, HBM_BEST = 8.0e12, 4.3e12


def data(N):
    rs = np.random.RandomState(0)
    x = rs.rand(N, 1) * 2 * np.pi - np.pi
    return x, 0.02 * rs.randn(N, 1) + np.sin(x)


def rate(eng, n, ini, warm):
    eng.run(warm, ini, store_chain=False)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    eng.run(n, ini, store_chain=False)
    torch.cuda.synchronize()
    return n / (time.perf_counter() - t0)


def step_kernel_us(C, p, alpha, reps=400):
    """qn_sg_step alone on [C, p] float64, nothing stored: microseconds per launch (device events) and bytes per launch."""
    L, dev, f64 = _lib.lib(), "cuda", torch.float64
    th, v, g = (torch.zeros(C, p, dtype=f64, device=dev) for _ in range(3))
    sse, best, best_lp = torch.zeros(C, dtype=f64, device=dev), torch.zeros(C, p, dtype=f64, device=dev), torch.zeros(2, C, dtype=f64, device=dev)
    lps, st = torch.zeros(C, 2, dtype=f64, device=dev), torch.ones(2, dtype=torch.int64, device=dev)     # t = 1, thin = 1 << 30: no trace
    call = lambda par: _lib.check(L.qn_sg_step(th.data_ptr(), v.data_ptr() if alpha != 1.0 else None, g.data_ptr(), _lib.QN_F64,
                                               sse.data_ptr(), 0.02, 4096, 512, 1e-9, alpha, 1.0, 0, 0, 0.0, 1 << 30, 0, C, 0, p, 1, 1,
                                               None, best.data_ptr(), best_lp.data_ptr(), None, lps.data_ptr(), None, st.data_ptr(),
                                               par, None), "qn_sg_step")
    for i in range(20):
        call(i & 1)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(reps):
        call(i & 1)
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps, C * p * (40 if alpha != 1.0 else 24)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sgmcmc.txt"))
    ap.add_argument("--cfg2-only", action="store_true")
    a = ap.parse_args()
    lines = ["device SGHMC (alpha = 0.1, eta = 1e-9, thin = 1, chain not stored), %s" % torch.cuda.get_device_name(0),
             "inner steps/s = gradient launches/s; DeviceMALA: one full-data gradient per step (HMC, L = 1)", ""]
    shapes = [("cfg2", (1, 64, 64, 64, 1), 4096, 64, 400, 300), ("cfg5", (1, 256, 256, 256, 256, 1), 32768, 256, 40, 3)]
    for name, dims, N, C, nmini, nfull in shapes[:1 if a.cfg2_only else 2]:
        arch = MLPArch(dims, "tanh")
        x, y = data(N)
        op = BatchedMLP(arch, x, y)
        ini = np.stack([0.1 * np.random.RandomState(1000 + c).randn(arch.nparams) for c in range(C)])
        lines.append("%s: %d chains, p = %d, N = %d" % (name, C, arch.nparams, N))
        for batch in (512, 2048, None):
            n = nfull if batch is None else nmini
            for graph in (False, True):
                r = rate(DeviceSGHMC(op, 0.02, eta=1e-9, alpha=0.1, batch=batch, seed=1, use_graph=graph), n, ini, max(4, n // 5))
                lines.append("  SGHMC batch %-5s %s  %10.2f inner steps/s" % (batch or "all", "graph " if graph else "direct", r))
        r = rate(DeviceMALA(op, 0.02, epsilon=1e-7, seed=1), nfull, ini, max(4, nfull // 5))
        lines.append("  DeviceMALA (L = 1, all rows)       %10.2f steps/s" % r)
        for alpha, label in ((0.1, "SGHMC"), (1.0, "SGLD ")):
            us, nbytes = step_kernel_us(C, arch.nparams, alpha)
            lines.append("  qn_sg_step alone, %s: %.2f us per launch, %.2f MB -> %.2f TB/s; traffic bound %.2f us at %.1f TB/s (peak), "
                         "%.2f us at %.1f TB/s (best measured stream)" % (label, us, nbytes / 1e6, nbytes / us / 1e6, nbytes / HBM_PEAK * 1e6,
                                                                         HBM_PEAK / 1e12, nbytes / HBM_BEST * 1e6, HBM_BEST / 1e12))
        lines.append("")
        del op
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
