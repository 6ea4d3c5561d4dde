#!/usr/bin/env python3
"""Gauss-Newton curvature and linearised predictive on the MI355X: 8 members of the 3x64 tanh network (d = 1, p = 8513),
N = 4096 rows.

    python tools/bench_glm.py [--reps 3] [--no-host] [--no-torch] [--out profiles/laplace_glm.txt]

* qn_mlp_curv GGN_FULL beside HESS_FULL in the same run; algorithmic rate against B o p (p + 1) N flop.
* qn_mlp_glm_predict (dense Sigma) against 2 B N o p^2 flop, and the diagonal kind as a time.
* the torch route on the same GPU: vmap(jacrev) Jacobians (J materialised) plus a float64 einsum, member by member.
* one member's np.linalg.svd on the host: what the sampled predictive pays per member and the closed form does not.
Rates are against the 78.6 TFLOP/s float64 MFMA peak.  One warm-up call, then the median of the reps.
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


def torch_net(arch):
    def f(w, xn):
        h, off = xn, 0
        L = len(arch.dims) - 1
        for i, (a, b) in enumerate(zip(arch.dims[:-1], arch.dims[1:])):
            h = w[off:off + a * b].view(b, a) @ h + w[off + a * b:off + a * b + b]
            off += a * b + b
            if i + 1 < L:
                h = torch.tanh(h)
        return h
    return f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--members", type=int, default=8)
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def emit(d):
        s = json.dumps(d)
        print(s, flush=True)
        lines.append(s)

    arch = MLPArch((1, 64, 64, 64, 1), "tanh")
    p, N, B, o = arch.nparams, a.rows, a.members, 1
    rs = np.random.RandomState(0)
    x = rs.rand(N, 1) * 2 - 1
    y = np.sin(3 * x) + 0.05 * rs.randn(N, 1)
    W = rs.randn(B, p) / 8
    op = BatchedMLP(arch, x, y, device="cuda:0")
    Wd = op.weights(W)
    shape = "%d x (1,64,64,64,1) tanh, N=%d, p=%d" % (B, N, p)
    t_ggn, ts_ggn = gpu_time(lambda: op.curvature(Wd, "ggn"), a.reps)
    t_full, ts_full = gpu_time(lambda: op.curvature(Wd, "full"), a.reps)
    t_gd, ts_gd = gpu_time(lambda: op.curvature(Wd, "ggn_diag"), a.reps)
    flops = B * o * p * (p + 1) * N
    emit(dict(what="qn_mlp_curv", shape=shape, ggn_full_s=t_ggn, ggn_full_runs_s=ts_ggn, hess_full_s=t_full,
              hess_full_runs_s=ts_full, ggn_over_hess=t_ggn / t_full, ggn_diag_s=t_gd, ggn_diag_runs_s=ts_gd,
              ggn_yardstick="B * o * p * (p + 1) * N = %.4g flop" % flops, ggn_tflops=flops / t_ggn / 1e12,
              ggn_frac_of_f64_mfma_peak=flops / t_ggn / PEAK_F64))
    # a well-conditioned SPD Sigma per member, made on the device
    g = torch.Generator(device="cuda:0").manual_seed(1)
    Sig = torch.empty(B, p, p, dtype=torch.float64, device="cuda:0")
    for b in range(B):
        A = torch.randn(p, p, dtype=torch.float64, device="cuda:0", generator=g) / np.sqrt(p)
        Sig[b] = A @ A.T + 0.5 * torch.eye(p, dtype=torch.float64, device="cuda:0")
    del A
    t_glm, ts_glm = gpu_time(lambda: op.glm_predict(Wd, Sig), a.reps)
    t_gld, ts_gld = gpu_time(lambda: op.glm_predict(Wd, Sig[:, 0, :].abs().contiguous()), a.reps)
    gflops = 2 * B * N * o * p * p
    rec = dict(what="qn_mlp_glm_predict", shape=shape, glm_full_s=t_glm, glm_full_runs_s=ts_glm,
               glm_yardstick="2 * B * N * o * p^2 = %.4g flop" % gflops, glm_tflops=gflops / t_glm / 1e12,
               glm_frac_of_f64_mfma_peak=gflops / t_glm / PEAK_F64, glm_diag_s=t_gld, glm_diag_runs_s=ts_gld)
    if not a.no_torch:
        f = torch_net(arch)
        jac = torch.func.vmap(torch.func.jacrev(f), in_dims=(None, 0))
        X = op.X

        def torch_route():
            out = []
            for b in range(B):
                J = jac(Wd[b], X)[:, 0, :]                      # [N, p], materialised
                out.append(torch.einsum("np,pq,nq->n", J, Sig[b], J))
            return torch.stack(out)
        t_t, ts_t = gpu_time(torch_route, a.reps)
        ref = torch_route()
        got = op.glm_predict(Wd, Sig)[1][:, :, 0, 0]
        rec.update(torch_route_s=t_t, torch_route_runs_s=ts_t, torch_over_kernel=t_t / t_glm,
                   max_rel_diff_vs_torch=float(((got - ref).abs() / ref.abs()).max()))
    emit(rec)
    if not a.no_host:
        C = Sig[0].cpu().numpy()
        t0 = time.perf_counter(); np.linalg.svd(C); t_svd = time.perf_counter() - t0
        emit(dict(what="host np.linalg.svd of one member's covariance", p=p, host_svd_s=t_svd,
                  host_threads=os.environ.get("OMP_NUM_THREADS")))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("# tools/bench_glm.py --reps %d: %s\n" % (a.reps, shape))
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
