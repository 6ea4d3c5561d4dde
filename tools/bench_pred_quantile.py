#!/usr/bin/env python3
"""qn_pred_quantile (csrc/qn_quantile.hip) on the MI355X: mixture mode timed alternately with the SCORE_PIT streaming pass of
qn_pred_score on the same arrays (one pass over the members; a quantile call is one pass per evaluation), empirical mode
alternately with torch.sort of the same tensor along the members on the same card (what torch.quantile does first; torch.quantile
itself refuses more than 16 million elements).

    python tools/bench_pred_quantile.py [--reps 3] [--windows 5] [--ms 256 1024 4096] [--out profiles/pred_quantile.txt]

Shapes: K = 32768 entries, M members, float64 F around 0 with spread 1, sigma = 0.5, no V, equal weights; Q in {1, 3, 9} levels
spread evenly over (0.05, 0.95) (the median alone for Q = 1).  Per (M, Q) one JSON line: the seconds of each pass (device-event
times of `reps` back-to-back calls after a warm-up call that also settles the clock, the passes alternating window by window,
median over `windows`) and the mean and the largest entry of `iters`."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from quinn_amd import _lib, scoring                              # noqa: E402

K = 32768
QS = (1, 3, 9)
SIGMA = 0.5


def window_time(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / 1e3 / reps


def bench_shape(M, Q, reps, windows):
    F = torch.randn(M, K, dtype=torch.float64, device="cuda")
    y = torch.randn(K, dtype=torch.float64, device="cuda")
    q = [0.5] if Q == 1 else list(np.linspace(0.05, 0.95, Q))
    qt = torch.as_tensor(q, dtype=torch.float64, device="cuda")
    iters = {}

    def mix():
        iters["it"] = scoring.quantile_rows(F, q, SIGMA, return_iters=True)[1]

    def pit():
        scoring.score_rows(F, y, SIGMA, None, _lib.SCORE_PIT)

    def emp():
        scoring.quantile_rows(F, q, 0.0)

    def tq():
        torch.sort(F, dim=0)

    for fn in (mix, pit, emp, tq):                               # warm-up: the LDS attribute, the allocator, the clock
        fn()
    torch.cuda.synchronize()
    t = {name: [] for name in ("mix", "pit", "emp", "tq")}
    for _ in range(windows):                                     # alternately, so a drifting clock hits all alike
        for name, fn in (("mix", mix), ("pit", pit), ("emp", emp), ("tq", tq)):
            t[name].append(window_time(fn, reps))
    it = iters["it"].double()
    head = F[:, :1024].contiguous()                               # torch.quantile's size limit: a slice of the entries
    same = bool(torch.allclose(scoring.quantile_rows(head, q, 0.0), torch.quantile(head, qt, dim=0), rtol=1e-14, atol=0.0))
    return dict(M=M, K=K, Q=Q, mixture_s=float(np.median(t["mix"])), mixture_runs_s=t["mix"], score_pit_s=float(np.median(t["pit"])),
                score_pit_runs_s=t["pit"], iters_mean=float(it.mean()), iters_max=int(it.max()), empirical_s=float(np.median(t["emp"])),
                empirical_runs_s=t["emp"], torch_sort_s=float(np.median(t["tq"])), torch_sort_runs_s=t["tq"],
                empirical_matches_torch_quantile=same)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--ms", type=int, nargs="+", default=[256, 1024, 4096])
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pred_quantile.py measures on the GPU; none is visible")
    lines = [dict(device=torch.cuda.get_device_name(0), reps=a.reps, windows=a.windows, sigma=SIGMA)]
    print(json.dumps(lines[0]), flush=True)
    for M in a.ms:
        for Q in QS:
            lines.append(bench_shape(M, Q, a.reps, a.windows))
            print(json.dumps(lines[-1]), flush=True)
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
