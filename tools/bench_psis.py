#!/usr/bin/env python3
"""qn_psis_loo (csrc/qn_psis.hip) on the MI355X beside the streaming pass of qn_pred_score on the same arrays.

    python tools/bench_psis.py [--reps 3] [--windows 5] [--out profiles/psis_loo.txt]
    python tools/bench_psis.py --one M K        (one shape in this process; what the line above starts per shape)

Shapes: M = 256, 1024, 4096 members x K = 32768 entries, float64 and float32 F, no V.  Every shape runs in a child process of
its own under a time limit, and the first child that fails ends the run.

  psis     one qn_psis_loo call: three launches (ratio maximum, tail selection and Pareto fit, rows).
  stream   one qn_pred_score call with what = LPPD | PWAIC: the streaming kernel alone, the yardstick -- one pass over F.
The two are timed alternately in one process: window i times `reps` back-to-back calls of one, then of the other, with device
events, after a warm-up call of each; the medians over the windows and their ratio are reported.
  bytes    requested by the kernels' loads and stores, against the M K elements of F: qn_psis_loo reads F three times (the
           tail pass in rows of 4 entries, 32 bytes of float64 or 16 of float32, which the memory system serves in larger
           lines -- the requested figure is a lower bound of the traffic), T tail members per entry once more by index, Y
           three times, and writes and reads its [10, K] workspace and the 4 rows.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from quinn_amd import _lib, psis                                 # noqa: E402

MS, K0 = (256, 1024, 4096), 32768
STREAM = _lib.SCORE_LPPD | _lib.SCORE_PWAIC


def window(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / 1e3 / reps


def bench_one(M, K, reps, windows):
    L = _lib.lib()
    st = _lib.stream()
    gen = torch.Generator(device="cuda").manual_seed(M * 100003 + K)
    mu = torch.randn(K, dtype=torch.float64, device="cuda", generator=gen)
    y = mu + 0.7 * torch.randn(K, dtype=torch.float64, device="cuda", generator=gen)
    out = torch.empty(_lib.SCORE_NOUT, K, dtype=torch.float64, device="cuda")
    loo = torch.empty(_lib.LOO_NOUT, K, dtype=torch.float64, device="cuda")
    need = int(L.qn_psis_loo_workspace_bytes(M, K))
    ws = torch.empty(need // 8, dtype=torch.float64, device="cuda")
    need_s = int(L.qn_pred_score_workspace_bytes(M, K, STREAM))
    T = psis.tail_size(M)
    lines = []
    for tdt, qdt, esz in ((torch.float64, _lib.QN_F64, 8), (torch.float32, _lib.QN_F32, 4)):
        F = (mu + 0.5 * torch.randn(M, K, dtype=torch.float64, device="cuda", generator=gen)).to(tdt).contiguous()

        def f_psis():
            _lib.check(L.qn_psis_loo(F.data_ptr(), None, qdt, y.data_ptr(), M, K, 0.7, loo.data_ptr(), ws.data_ptr(), need, st),
                       "qn_psis_loo")

        def f_stream():
            _lib.check(L.qn_pred_score(F.data_ptr(), None, qdt, y.data_ptr(), M, K, 0.7, STREAM, out.data_ptr(), ws.data_ptr(),
                                       need_s, st), "qn_pred_score")

        f_psis()
        f_stream()
        torch.cuda.synchronize()
        tp, ts = [], []
        for _ in range(windows):
            tp.append(window(f_psis, reps))
            ts.append(window(f_stream, reps))
        t_p, t_s = float(np.median(tp)), float(np.median(ts))
        elem = M * K * esz
        nb = 3 * elem + T * K * esz + 3 * K * 8 + (1 + 9 + 10) * K * 8 + 4 * K * 8
        khat = loo[1]
        lines.append(dict(M=M, K=K, T=T, dtype=str(tdt).split(".")[1], psis_s=t_p, stream_s=t_s, psis_over_stream=t_p / t_s,
                          F_bytes=elem, psis_bytes_requested=nb, bytes_over_F=nb / elem, psis_TBps_requested=nb / t_p / 1e12,
                          stream_TBps=(elem + 3 * K * 8) / t_s / 1e12, finite=bool(torch.isfinite(loo[[0, 2, 3]]).all()),
                          khat_median=float(khat.median()), khat_above_0p7=float((khat > 0.7).double().mean())))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--one", type=int, nargs=2, metavar=("M", "K"), default=None)
    ap.add_argument("--step-timeout", type=int, default=150, help="seconds a shape's child process may take")
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file (replaced)")
    a = ap.parse_args()
    if a.one:
        if not torch.cuda.is_available():
            raise SystemExit("bench_psis.py measures on the GPU; none is visible")
        for ln in bench_one(a.one[0], a.one[1], a.reps, a.windows):
            print(json.dumps(ln), flush=True)
        return
    lines = []
    for M in MS:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", str(M), str(K0), "--reps", str(a.reps),
                            "--windows", str(a.windows)], capture_output=True, text=True, timeout=a.step_timeout)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        if r.returncode != 0:
            raise SystemExit(f"M={M} K={K0}: exit {r.returncode}\n{r.stderr[-2000:]}")
        lines += [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for ln in lines:
                f.write(ln + "\n")


if __name__ == "__main__":
    main()
