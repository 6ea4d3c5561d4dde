#!/usr/bin/env python3
"""SWAG on the MI355X: the fused moment pass qn_swag_step, one whole SWAG step (gradient + collect) against the gradient
alone, and the posterior draws of qn_swag_sample.

    python tools/bench_swag.py [--cfg cfg2 cfg4] [--reps 20] [--draws 100]

  cfg2   64 members of the (1,64,64,64,1) tanh network, N = 4096 rows (p = 8,513)
  cfg4   512 members of the (1,256,256,256,256,1) tanh network, N = 16384 rows (p = 198,145)

qn_swag_step (collecting, K = 10 deviation rows) moves 64 B per parameter per member: W, G, m1, m2 read, W, m1, m2 and one
deviation row written (float64).  Its rate is reported against the ~6.3 TB/s achievable HBM bandwidth (MI355X_MICROARCH.md).
Times are CUDA-event times of `reps` back-to-back calls after a warm-up, median of 3 such windows.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from quinn_amd import _lib                                       # noqa: E402
from quinn_amd.ops import MLPArch, BatchedMLP, swag_step, swag_sample   # noqa: E402

HBM_ACHIEVABLE = 6.3e12
CFGS = {"cfg2": (64, (1, 64, 64, 64, 1), 4096), "cfg4": (512, (1, 256, 256, 256, 256, 1), 16384)}


def timed(fn, reps, windows=3):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / 1e3 / reps)
    return float(np.median(out)), out


def bench(name, reps, draws):
    B, dims, N = CFGS[name]
    arch = MLPArch(dims, "tanh")
    p, K, dev = arch.nparams, 10, "cuda:0"
    rs = np.random.RandomState(0)
    x = rs.rand(N, 1) * 2 - 1
    y = np.sin(3 * x) + 0.05 * rs.randn(N, 1)
    op = BatchedMLP(arch, x, y, device=dev)
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    W = torch.randn(B, p, dtype=torch.float64, device=dev, generator=g) / 16
    m1, m2 = torch.empty_like(W), torch.empty_like(W)
    D = torch.zeros(B, K, p, dtype=torch.float64, device=dev)
    lr = torch.full((B,), 1e-6, dtype=torch.float64, device=dev)
    sse = torch.empty(B, dtype=torch.float64, device=dev)
    G = torch.empty(B, p, dtype=torch.float64, device=dev)
    swag_step(_lib.SWAG_INIT, W, m1=m1, m2=m2)
    op.sse_grad(W, out=(sse, G))
    gscale = 1.0 / N
    state = {"n": 0}

    def collect():
        state["n"] += 1
        swag_step(_lib.SWAG_SGD_COLLECT, W, G, lr, gscale, m1, m2, D, slot=(state["n"] - 1) % K, n=state["n"])

    def grad():
        op.sse_grad(W, out=(sse, G))

    def step():
        grad()
        collect()

    t_col, runs_col = timed(collect, reps)
    nbytes = 64 * B * p
    t_grad, runs_grad = timed(grad, max(1, reps // 10))
    t_step, runs_step = timed(step, max(1, reps // 10))
    out = dict(cfg=name, members=B, dims=list(dims), N=N, p=p, K=K,
               collect_s=t_col, collect_runs_s=runs_col, collect_bytes=nbytes, collect_GBps=nbytes / t_col / 1e9,
               collect_frac_of_achievable_hbm=nbytes / t_col / HBM_ACHIEVABLE,
               grad_s=t_grad, step_s=t_step, step_over_grad=t_step / t_grad, grad_runs_s=runs_grad, step_runs_s=runs_step,
               finite=bool(torch.isfinite(m1).all() and torch.isfinite(D).all()))
    # posterior draws: `draws` samples spread over the members, inputs already on the device
    diag = (m2 - m1 * m1).abs()
    js = rs.randint(0, B, draws)
    z1 = torch.randn(draws, p, dtype=torch.float64, device=dev, generator=g)
    z2 = torch.randn(draws, K, dtype=torch.float64, device=dev, generator=g)
    theta = torch.empty(draws, p, dtype=torch.float64, device=dev)
    mean = m1.clone()
    for drift in (1, 0):
        t, runs = timed(lambda: swag_sample(mean, diag, D, js, z1, z2, drift, theta=theta), max(1, reps // 4))
        sbytes = draws * p * 8 * (K + 3 + 2 * drift)          # D rows, diag, z1, theta (+ mean read / write with drift)
        out[f"sample_drift{drift}_s"] = t
        out[f"sample_drift{drift}_GBps"] = sbytes / t / 1e9
    out["sample_draws"] = draws
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cfg", nargs="+", default=["cfg2", "cfg4"], choices=sorted(CFGS))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--draws", type=int, default=100)
    a = ap.parse_args()
    for name in a.cfg:
        print(json.dumps(bench(name, a.reps, a.draws)), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
