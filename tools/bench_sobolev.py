#!/usr/bin/env python3
"""Input Jacobian and derivative-informed loss on the MI355X: `BatchedMLP.sobolev(want_grad=True)` and `input_jacobian`.

    python tools/bench_sobolev.py [--reps 5] [--members 64] [--rows 4096] [--no-torch] [--out profiles/sobolev.txt]

Shapes: 64 members x 3x64 tanh x N = 4096 for d = 2, 6, 12, and a 4x256 tanh network at d = 6.  In the same process on the
same card, per shape:
* (a) the same loss by torch autograd on the GPU in float64: vmap(jacrev) over the rows under autograd.grad, vmapped over
  the members -- the only route to the quantity without the kernels; the weight gradients of the two routes are compared.
* (b) the project's plain-float64 gradient, `use_exact_float64()` `sse_grad`, on a dataset of (1 + d) N rows: the same
  matrix-product flops without the tangent bookkeeping.
Algorithmic flop of the loss gradient: the three products of `MLPArch.flops_fwdbwd` over (1 + d) N extended rows per member;
rates are whole-call rates (all launches of the call) against the 78.6 TFLOP/s float64 MFMA peak.  Two warm-up calls, then
the median of the reps, each timed by a host clock around a device synchronise.
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


def gpu_time(fn, reps, warm=2):
    for _ in range(warm):
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--members", type=int, default=64)
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--torch-members", type=int, default=8, help="members per vmap call of the torch route (memory)")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sobolev.py needs the GPU; there is no CPU fallback")
    lines = []

    def emit(d):
        s = json.dumps(d)
        print(s, flush=True)
        lines.append(s)

    B, N = a.members, a.rows
    shapes = [((d, 64, 64, 64, 1), B) for d in (2, 6, 12)] + [((6, 256, 256, 256, 256, 1), B)]
    for dims, Bm in shapes:
        arch = MLPArch(dims, "tanh")
        d, p = dims[0], arch.nparams
        rs = np.random.RandomState(d)
        x = rs.rand(N, d) * 2 - 1
        y = np.sin(x.sum(1, keepdims=True))
        g = np.cos(x.sum(1, keepdims=True)) * np.ones((1, d))
        W = rs.randn(Bm, p) / np.sqrt(max(dims))
        op = BatchedMLP(arch, x, y, device="cuda:0")
        op.set_grad_data(g)
        Wd = op.weights(W)
        wv, wg = 1.0 / N, 0.5 / (N * d)
        t_sob, ts_sob = gpu_time(lambda: op.sobolev(Wd, wv, wg), a.reps)
        t_val, ts_val = gpu_time(lambda: op.sobolev(Wd, wv, wg, want_grad=False), a.reps)
        t_jac, ts_jac = gpu_time(lambda: op.input_jacobian(Wd), a.reps)
        S = 1 + d
        flops = Bm * arch.flops_fwdbwd(S * N)
        rec = dict(what="sobolev", shape="%d x %s tanh, N=%d, p=%d" % (Bm, dims, N, p), sobolev_grad_s=t_sob,
                   sobolev_grad_runs_s=ts_sob, sobolev_values_s=t_val, sobolev_values_runs_s=ts_val, input_jacobian_s=t_jac,
                   input_jacobian_runs_s=ts_jac, yardstick="B * flops_fwdbwd((1 + d) N) = %.4g flop" % flops,
                   sobolev_grad_tflops=flops / t_sob / 1e12, sobolev_grad_frac_of_f64_mfma_peak=flops / t_sob / PEAK_F64,
                   input_jacobian_tflops=Bm * arch.flops_fwd(S * N) / t_jac / 1e12)
        # (b) the plain-float64 gradient on (1 + d) N rows
        xe = np.tile(x, (S, 1))
        ope = BatchedMLP(arch, xe, np.tile(y, (S, 1)), device="cuda:0")
        rec["sse_grad_path"] = ope.use_exact_float64()
        t_b, ts_b = gpu_time(lambda: ope.sse_grad(Wd), a.reps)
        rec.update(sse_grad_ext_rows_s=t_b, sse_grad_ext_rows_runs_s=ts_b, sobolev_over_sse_grad=t_sob / t_b)
        del ope
        # (a) torch autograd on the same card
        if not a.no_torch:
            f = torch_net(arch)
            X, Y, G = op.X, op.Y, op.G

            def loss_one(w):
                pred = torch.func.vmap(f, in_dims=(None, 0))(w, X)
                J = torch.func.vmap(torch.func.jacrev(f, argnums=1), in_dims=(None, 0))(w, X)
                return wv * ((pred - Y) ** 2).sum() + wg * ((J - G) ** 2).sum()

            grad_members = torch.func.vmap(torch.func.grad(loss_one))
            tb = max(1, min(a.torch_members, Bm))

            def torch_route():
                return torch.cat([grad_members(Wd[b0:b0 + tb]) for b0 in range(0, Bm, tb)])
            try:
                t_t, ts_t = gpu_time(torch_route, max(2, a.reps // 2), warm=1)
                ref = torch_route()
                got = op.sobolev(Wd, wv, wg)[2]
                rec.update(torch_autograd_s=t_t, torch_autograd_runs_s=ts_t, torch_over_sobolev=t_t / t_sob,
                           torch_members_per_call=tb,
                           max_grad_diff_vs_torch=float((got - ref).abs().max() / ref.abs().max()))
                del ref, got
            except torch.OutOfMemoryError as e:
                rec.update(torch_autograd_s=None, torch_autograd_error="out of memory: " + str(e)[:80])
            torch.cuda.empty_cache()
        emit(rec)
        del op
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("# tools/bench_sobolev.py --reps %d --members %d --rows %d\n" % (a.reps, B, N))
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
