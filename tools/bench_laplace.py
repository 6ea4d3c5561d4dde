#!/usr/bin/env python3
"""Laplace curvature on the MI355X: qn_mlp_curv for 8 members of the 3x64 tanh network (d = 1, p = 8513) on N = 4096
rows, both kinds, and the host-side inverse / SVD of one p x p matrix that NN_Laplace does on top.

    python tools/bench_laplace.py [--reps 3] [--no-host] [--reference DIR]

Algorithmic rate of FULL: the yardstick is p (p + 1) N flops per member (the useful multiply-adds of assembling the p x p
Hessian over N rows, the tangents not counted), against the 78.6 TFLOP/s float64 MFMA peak.  DIAG is reported as time
only.  --reference DIR also times the reference's la_calc Hessian (one autograd pass per parameter, CPU) at the size of
the g14_laplace fixture (p = 97, 24 rows), where its package is importable.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from quinn_amd.ops import MLPArch, BatchedMLP    # noqa: E402

PEAK_F64 = 78.6e12


def gpu_time(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--members", type=int, default=8)
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--reference", default=None)
    a = ap.parse_args()
    out = {}
    if a.reference is None:
        arch = MLPArch((1, 64, 64, 64, 1), "tanh")
        p, N, B = arch.nparams, a.rows, a.members
        rs = np.random.RandomState(0)
        x = rs.rand(N, 1) * 2 - 1
        y = np.sin(3 * x) + 0.05 * rs.randn(N, 1)
        W = rs.randn(B, p) / 8
        op = BatchedMLP(arch, x, y, device="cuda:0")
        Wd = op.weights(W)
        t_full, ts_full = gpu_time(lambda: op.curvature(Wd, "full"), a.reps)
        t_diag, ts_diag = gpu_time(lambda: op.curvature(Wd, "diag"), a.reps)
        H = op.curvature(Wd[:2], "full")
        finite, symmetric = bool(torch.isfinite(H).all()), bool(torch.equal(H, H.transpose(1, 2)))
        del H
        flops = B * p * (p + 1) * N
        out.update(shape="8 x (1,64,64,64,1) tanh, N=%d, p=%d" % (N, p), members=B, full_s=t_full, full_runs_s=ts_full,
                   full_tflops=flops / t_full / 1e12, full_frac_of_f64_mfma_peak=flops / t_full / PEAK_F64,
                   full_yardstick="B * p * (p + 1) * N = %.4g flop" % flops, diag_s=t_diag, diag_runs_s=ts_diag,
                   full_ms_per_member=1e3 * t_full / B, diag_ms_per_member=1e3 * t_diag / B, full_finite=finite, full_symmetric=symmetric)
        print(json.dumps(out), flush=True)
        if not a.no_host:            # a well-conditioned SPD stand-in of the same size (the Hessian itself may be indefinite)
            A = rs.randn(p, p)
            S = A @ A.T / p + np.eye(p)
            t0 = time.perf_counter(); C = np.linalg.inv(S); t_inv = time.perf_counter() - t0
            t0 = time.perf_counter(); np.linalg.svd(C); t_svd = time.perf_counter() - t0
            out = dict(p=p, host_inv_s=t_inv, host_svd_s=t_svd, host_threads=os.environ.get("OMP_NUM_THREADS"))
    else:
        sys.path.insert(0, a.reference)
        from quinn.nns.mlp import MLP
        from quinn.nns.nnwrap import NNWrap
        from quinn.nns.losses import NegLogPost
        torch.set_default_dtype(torch.double)
        torch.manual_seed(150)
        net = MLP(1, 1, (8, 8), activ="tanh")
        rs = np.random.RandomState(1)
        x, y = rs.randn(24, 1), rs.randn(24, 1)
        nw = NNWrap(net)
        w = nw.p_flatten().detach().numpy().flatten()
        loss = NegLogPost(net, 24, 0.1, None)
        t0 = time.perf_counter(); nw.calc_hess_full(w, loss, x, y); t_f = time.perf_counter() - t0
        t0 = time.perf_counter(); nw.calc_hess_diag(w, loss, x, y); t_d = time.perf_counter() - t0
        out.update(reference_la_calc_full_s=t_f, reference_la_calc_diag_s=t_d, reference_shape="(1,8,8,1) tanh, p=97, 24 rows, CPU")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
