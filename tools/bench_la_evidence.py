#!/usr/bin/env python3
"""The Laplace-evidence kernels (csrc/qn_evidence.hip) on the MI355X beside a torch route on the same card.

    python tools/bench_la_evidence.py [--reps 3] [--windows 5] [--iters 50] [--out profiles/la_evidence.txt]

One JSON line per measurement.  Each pair is timed alternately in one process after a warm-up call of each: window i times
`reps` back-to-back calls of one, then of the other, with device events; the medians over the windows are reported.
Shapes: the parameter counts of cfg2 (3x64, p = 8513, G = 4 layers) and cfg4 (4x256, p = 198145, G = 5 layers) with B = 64 and
512 members, and B = 1 at both -- a member is ONE workgroup of 256 threads on one CU, so a single member uses 1 / 256 of the card.
  evidence    qn_la_evidence (Hc = 1) beside torch: lam = c / s2 + tau, lam.log().sum(-1), the per-group sums of (c / s2) / lam
              and of w^2.
  tune_iter   one iterate of qn_la_tune, timed as a call with tol = 0 and max_iter = `iters` divided by the iterates the slowest
              member evaluated (`iterates`: the fixed point can be met bit for bit, resid = 0, before `iters`), beside the same torch expressions without the w^2 sums (one iterate's logdet and gamma_g; the update is not counted).
`elems_per_s` is B p elements per second of the kernel -- one division, one log and a few multiply-adds per element.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from quinn_amd import evidence as ev                             # noqa: E402

SHAPES = {"cfg2": (8513, (0, 128, 4288, 8448, 8513)), "cfg4": (198145, (0, 512, 66304, 132096, 197888, 198145))}


def window(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / 1e3 / reps


def alternate(fa, fb, reps, windows):
    fa()
    fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(windows):
        ta.append(window(fa, reps))
        tb.append(window(fb, reps))
    return float(np.median(ta)), float(np.median(tb))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file (replaced)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_la_evidence.py measures on the GPU; none is visible")
    lines = []

    def emit(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    for name, (p, bounds) in SHAPES.items():
        bounds = np.asarray(bounds, dtype=np.int64)
        G, n = len(bounds) - 1, 10 * p
        sizes = [int(s) for s in np.diff(bounds)]
        for B in (1, 64, 512):
            gen = torch.Generator(device="cuda").manual_seed(B + p)
            c = torch.exp(2.0 * torch.randn(B, p, dtype=torch.float64, device="cuda", generator=gen) + 1.0)
            W = 0.5 * torch.randn(B, p, dtype=torch.float64, device="cuda", generator=gen)
            sse = torch.full((B,), 0.01 * n, dtype=torch.float64, device="cuda")
            s2 = torch.full((B,), 0.09, dtype=torch.float64, device="cuda")
            tau = torch.ones(B, G, dtype=torch.float64, device="cuda")
            s2g, taug = s2[:, None].contiguous(), tau[:, None].contiguous()

            def torch_iter(with_s):
                q = c / s2[:, None]
                lam = q + torch.repeat_interleave(tau, torch.as_tensor(sizes, device="cuda"), dim=1, output_size=p)
                out = [lam.log().sum(-1)] + [r.sum(-1) for r in torch.split(q / lam, sizes, dim=1)]
                if with_s:
                    out += [r.sum(-1) for r in torch.split(W * W, sizes, dim=1)]
                return out

            tk, tt = alternate(lambda: ev.log_evidence_dev(c, W, sse, n, bounds, s2g, taug), lambda: torch_iter(True), a.reps, a.windows)
            emit(what="evidence", shape=name, p=p, G=G, B=B, kernel_s=tk, torch_s=tt, torch_over_kernel=tt / tk, elems_per_s=B * p / tk)
            res = ev.tune_dev(c, W, sse, n, bounds, s2, tau, tol=0.0, max_iter=a.iters)
            nit = int(res["status"][:, 0].max().item()) + 1      # the fixed point can be met bit for bit before `iters`
            tk, tt = alternate(lambda: ev.tune_dev(c, W, sse, n, bounds, s2, tau, tol=0.0, max_iter=a.iters), lambda: torch_iter(False),
                               a.reps, a.windows)
            tk /= nit
            emit(what="tune_iter", shape=name, p=p, G=G, B=B, iterates=nit, kernel_s=tk, torch_s=tt,
                 torch_over_kernel=tt / tk, elems_per_s=B * p / tk)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
