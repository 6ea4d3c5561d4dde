#!/usr/bin/env python3
"""qn_pred_score (csrc/qn_score.hip) alone on the MI355X: the streaming pass and the CRPS pair pass, per shape.

    python tools/bench_pred_score.py [--reps 5] [--windows 5] [--out profiles/pred_score.txt]
    python tools/bench_pred_score.py --one M K        (one shape in this process; what the line above starts per shape)

Shapes: M = 128, 1024 members x K = 4096, 32768 entries, float64 and float32, with and without V.  Every shape runs in a
child process of its own under a time limit, and the first child that fails ends the run.

  stream   a call with what = LPPD | PWAIC | PIT | MOMENTS: the streaming kernel alone.  Bytes = the M x K elements of F
           (and of V) read once + Y + the 5 rows written; bytes / time is set beside `qn_pred_moments` with variance on
           the same array (the existing kernel; it reads the array twice, and its bytes are counted twice).
  pair     time(all six rows) - time(stream): the pair kernel, plus the first CRPS sum of the streaming kernel and the
           finishing kernel, which are not separable through the C interface and are small beside it.  Pair evaluations =
           K M (M - 1) / 2 (the diagonal terms are closed forms); the Gaussian form (sigma > 0 or V) costs one exp and
           one erf each, the abs form (sigma = 0, V = NULL: time(CRPS | MOMENTS) - time(MOMENTS)) none.
Times are device-event times of `reps` back-to-back calls after a warm-up call, median over `windows` such windows.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from quinn_amd import _lib                                       # noqa: E402

MS, KS = (128, 1024), (4096, 32768)
STREAM = _lib.SCORE_LPPD | _lib.SCORE_PWAIC | _lib.SCORE_PIT | _lib.SCORE_MOMENTS
ALL = STREAM | _lib.SCORE_CRPS


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
    return float(np.median(out))


def bench_one(M, K, reps, windows):
    L = _lib.lib()
    st = _lib.stream()
    gen = torch.Generator(device="cuda").manual_seed(M * 100003 + K)
    mu = torch.randn(K, dtype=torch.float64, device="cuda", generator=gen)
    y = mu + 0.7 * torch.randn(K, dtype=torch.float64, device="cuda", generator=gen)
    out = torch.empty(_lib.SCORE_NOUT, K, dtype=torch.float64, device="cuda")
    need = int(L.qn_pred_score_workspace_bytes(M, K, ALL))
    ws = torch.empty(need // 8, dtype=torch.float64, device="cuda")
    lines = []
    for tdt, qdt, esz in ((torch.float64, _lib.QN_F64, 8), (torch.float32, _lib.QN_F32, 4)):
        F = (mu + 0.5 * torch.randn(M, K, dtype=torch.float64, device="cuda", generator=gen)).to(tdt).contiguous()
        Vd = (0.01 + 0.5 * torch.rand(M, K, dtype=torch.float64, device="cuda", generator=gen)).to(tdt).contiguous()

        def call(what, V, sigma):
            _lib.check(L.qn_pred_score(F.data_ptr(), V.data_ptr() if V is not None else None, qdt, y.data_ptr(), M, K,
                                       sigma, what, out.data_ptr(), ws.data_ptr(), need, st), "qn_pred_score")

        mean, var = out[4], out[5]
        t_mom = timed(lambda: _lib.check(L.qn_pred_moments(F.data_ptr(), qdt, M, K, mean.data_ptr(), var.data_ptr(), st),
                                         "qn_pred_moments"), reps, windows)
        pairs = K * M * (M - 1) // 2
        for V in (None, Vd):
            t_s = timed(lambda: call(STREAM, V, 0.3), reps, windows)
            t_a = timed(lambda: call(ALL, V, 0.3), reps, windows)
            nb = M * K * esz * (2 if V is not None else 1) + K * 8 + 5 * K * 8
            lines.append(dict(M=M, K=K, dtype=str(tdt).split(".")[1], V=V is not None, stream_s=t_s, stream_bytes=nb,
                              stream_TBps=nb / t_s / 1e12, pred_moments_s=t_mom,
                              pred_moments_TBps=(2 * M * K * esz + 2 * K * 8) / t_mom / 1e12, all_s=t_a,
                              pair_s=t_a - t_s, pair_evals=pairs, gauss_pairs_per_s=pairs / (t_a - t_s),
                              finite=bool(torch.isfinite(out).all())))
        t_m = timed(lambda: call(_lib.SCORE_MOMENTS, None, 0.0), reps, windows)
        t_c = timed(lambda: call(_lib.SCORE_MOMENTS | _lib.SCORE_CRPS, None, 0.0), reps, windows)
        lines.append(dict(M=M, K=K, dtype=str(tdt).split(".")[1], form="abs", moments_s=t_m, crps_moments_s=t_c,
                          pair_s=t_c - t_m, pair_evals=pairs, abs_pairs_per_s=pairs / (t_c - t_m)))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--one", type=int, nargs=2, metavar=("M", "K"), default=None)
    ap.add_argument("--step-timeout", type=int, default=150, help="seconds a shape's child process may take")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    if a.one:
        if not torch.cuda.is_available():
            raise SystemExit("bench_pred_score.py measures on the GPU; none is visible")
        for ln in bench_one(a.one[0], a.one[1], a.reps, a.windows):
            print(json.dumps(ln), flush=True)
        return
    lines = []
    for M in MS:
        for K in KS:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", str(M), str(K), "--reps", str(a.reps),
                                "--windows", str(a.windows)], capture_output=True, text=True, timeout=a.step_timeout)
            sys.stdout.write(r.stdout)
            sys.stdout.flush()
            if r.returncode != 0:
                raise SystemExit(f"M={M} K={K}: exit {r.returncode}\n{r.stderr[-2000:]}")
            lines += [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for ln in lines:
                f.write(ln + "\n")


if __name__ == "__main__":
    main()
