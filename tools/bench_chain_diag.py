#!/usr/bin/env python3
"""qn_chain_stats (csrc/qn_diag.hip) alone on the MI355X: time and bytes / time per shape, against a plain device copy
measured in the same run, and the host route (device-to-host copy + numpy) on a 4-chain slice for comparison.

    python tools/bench_chain_diag.py [--reps 5] [--windows 5] [--nburn-frac 0.5] [--small-only] [--out FILE]

Shapes [C, T, K]: the headline chain [64, 10001, 8513] float64 (43.6 GB), one chain of a small network [1, 10001, 321], the
log-posterior trace [64, 10001, 1] and a short prediction ensemble [64, 200, 4096]; nburn = T / 2 as fit(diagnostics=True)
uses (--nburn-frac 0: the whole chain).  Bytes = the window rows read once + the statistics written (the batch workspace's write and re-read are NOT
counted: they are overhead of the method).  Times are device-event times of `reps` back-to-back calls after a warm-up call,
median over `windows` such windows.  The yardstick is a float64 device-to-device copy (read + write bytes over its time)
of up to 8 GB in the same process; MI355X_MICROARCH.md gives ~6.3 TB/s for it.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from quinn_amd import _lib                                       # noqa: E402
from quinn_amd.mcmc import diagnostics as diag                   # noqa: E402

SHAPES = [(64, 10001, 8513), (1, 10001, 321), (64, 10001, 1), (64, 200, 4096)]


def timed(fn, reps, windows):
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


def copy_rate(reps, windows):
    n = (8 << 30) // 8
    src = torch.ones(n, dtype=torch.float64, device="cuda")
    dst = torch.empty_like(src)
    t, runs = timed(lambda: dst.copy_(src), reps, windows)
    del src, dst
    torch.cuda.empty_cache()
    return 2 * n * 8 / t, runs


def stats_np(chain, t0, nbatch, blen):
    """The [C, 6, K] statistics by numpy (two passes), the restatement the tests use."""
    C, T, K = chain.shape
    x = chain[:, t0:].reshape(2 * C, nbatch, blen, K)
    flat = x.reshape(2 * C, nbatch * blen, K)
    mean = flat.mean(axis=1)
    M2 = ((flat - mean[:, None]) ** 2).sum(axis=1)
    Sb = ((x.mean(axis=2) - mean[:, None]) ** 2).sum(axis=1)
    return np.concatenate([a.reshape(C, 2, K) for a in (mean, M2, Sb)], axis=1)


def bench_shape(shape, reps, windows, copy_bps, nburn_frac):
    C, T, K = shape
    x = torch.empty(C, T, K, dtype=torch.float64, device="cuda")
    for c in range(C):                                           # filled chain by chain: no second array of this size
        x[c].normal_()
    nburn = int(T * nburn_frac)
    t0, nbatch, blen = diag.batch_plan(T, nburn)
    L = _lib.lib()
    need = L.qn_chain_stats_workspace_bytes(C, T, K, nbatch, blen)
    ws = torch.empty(need // 8, dtype=torch.float64, device="cuda")
    stats = torch.empty(C, 6, K, dtype=torch.float64, device="cuda")
    st = _lib.stream()

    def call():
        _lib.check(L.qn_chain_stats(x.data_ptr(), _lib.QN_F64, C, T, K, t0, nbatch, blen, stats.data_ptr(), ws.data_ptr(),
                                    need, st), "qn_chain_stats")

    t, runs = timed(call, reps, windows)
    nbytes = C * (T - t0) * K * 8 + C * 6 * K * 8
    out = dict(shape=list(shape), t0=t0, nbatch=nbatch, blen=blen, seconds=t, runs_s=runs, bytes=nbytes,
               workspace_bytes=int(need), TBps=nbytes / t / 1e12, frac_of_copy=nbytes / t / copy_bps,
               finite=bool(torch.isfinite(stats).all()))
    if C >= 4:                                                   # the host route on a 4-chain slice
        torch.cuda.synchronize()
        h0 = time.perf_counter()
        host = x[:4].cpu().numpy()
        h1 = time.perf_counter()
        ref = stats_np(host, t0, nbatch, blen)
        h2 = time.perf_counter()
        t4, _ = timed(lambda: diag.chain_stats(x[:4], nburn), reps, windows)
        got = diag.chain_stats(x[:4], nburn).cpu().numpy()
        err = float(np.max(np.abs(got - ref) / np.max(np.abs(ref), axis=2, keepdims=True)))
        out.update(host4_copy_s=h1 - h0, host4_numpy_s=h2 - h1, device4_s=t4, host4_vs_device_max_rel=err)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--nburn-frac", type=float, default=0.5, help="burn-in as a fraction of T (0: the whole chain)")
    ap.add_argument("--small-only", action="store_true", help="skip the 43.6 GB shape")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_chain_diag.py measures on the GPU; none is visible")
    copy_bps, copy_runs = copy_rate(a.reps, a.windows)
    lines = [dict(device_copy_TBps=copy_bps / 1e12, device_copy_runs_s=copy_runs, device=torch.cuda.get_device_name(0))]
    print(json.dumps(lines[0]), flush=True)
    for shape in SHAPES:
        if a.small_only and shape[0] * shape[1] * shape[2] * 8 > (8 << 30):
            continue
        lines.append(bench_shape(shape, a.reps, a.windows, copy_bps, a.nburn_frac))
        print(json.dumps(lines[-1]), flush=True)
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
