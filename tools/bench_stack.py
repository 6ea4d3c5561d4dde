#!/usr/bin/env python3
"""The stacking kernels (csrc/qn_stack.hip) on the MI355X beside the kernels of qn_pred_score on the same arrays.

    python tools/bench_stack.py [--reps 3] [--windows 5] [--out profiles/stack.txt]

One JSON line per measurement.  Each pair is timed alternately in one process after a warm-up call of each: window i times
`reps` back-to-back calls of one, then of the other, with device events; the medians over the windows are reported.
  group_lpd   qn_group_lpd (G = 64 groups of 16, M = 1024, K = 32768, float64 F) beside qn_pred_score(LPPD): both stream F
              once; `bound_s` is the M K elements at 8 TB/s.
  stack_iter  one launch of qn_stack_weights' iteration (G = 64 and 512, K = 32768), timed as a call of `iters` launches that
              cannot stop (tol = 0) divided by iters; `bound_s` is the G K float64 of E at 8 TB/s -- E is read twice per
              launch (mix_k, then the sums over k), the second time from cache where a block's tile fits.
  score_w     qn_pred_score_w beside qn_pred_score at M = 256, K = 32768, with the pair pass (all rows) and without it.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from quinn_amd import _lib                                       # noqa: E402

K0, HBM = 32768, 8e12


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


def data(M, K, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    mu = torch.randn(K, dtype=torch.float64, device="cuda", generator=gen)
    y = mu + 0.7 * torch.randn(K, dtype=torch.float64, device="cuda", generator=gen)
    F = (mu + 0.5 * torch.randn(M, K, dtype=torch.float64, device="cuda", generator=gen)).contiguous()
    return F, y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file (replaced)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_stack.py measures on the GPU; none is visible")
    L, st = _lib.lib(), _lib.stream()
    lines = []

    def emit(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    # ---- qn_group_lpd beside the LPPD streaming pass
    M, G = 1024, 64
    F, y = data(M, K0, 1)
    off = np.arange(G + 1, dtype=np.int64) * (M // G)
    Lgk = torch.empty(G, K0, dtype=torch.float64, device="cuda")
    out = torch.empty(_lib.SCORE_NOUT, K0, dtype=torch.float64, device="cuda")
    need_g = int(L.qn_group_lpd_workspace_bytes(M, K0, G))
    need_s = int(L.qn_pred_score_workspace_bytes(M, K0, _lib.SCORE_LPPD))
    ws = torch.empty(max(need_g, need_s) // 8, dtype=torch.float64, device="cuda")
    t_g, t_s = alternate(
        lambda: _lib.check(L.qn_group_lpd(F.data_ptr(), None, _lib.QN_F64, y.data_ptr(), M, K0, 0.7, off.ctypes.data, G,
                                          Lgk.data_ptr(), ws.data_ptr(), need_g, st), "qn_group_lpd"),
        lambda: _lib.check(L.qn_pred_score(F.data_ptr(), None, _lib.QN_F64, y.data_ptr(), M, K0, 0.7, _lib.SCORE_LPPD,
                                           out.data_ptr(), ws.data_ptr(), need_s, st), "qn_pred_score"), a.reps, a.windows)
    emit(what="group_lpd", G=G, M=M, K=K0, group_lpd_s=t_g, pred_score_lppd_s=t_s, ratio=t_g / t_s, bound_s=M * K0 * 8 / HBM)

    # ---- one iteration of qn_stack_weights
    for G in (64, 512):
        gen = torch.Generator(device="cuda").manual_seed(G)
        Lr = -torch.rand(G, K0, dtype=torch.float64, device="cuda", generator=gen) * 3
        w = torch.empty(G, dtype=torch.float64, device="cuda")
        status = torch.empty(_lib.STACK_NSTATUS, dtype=torch.float64, device="cuda")
        need = int(L.qn_stack_weights_workspace_bytes(G, K0))
        wsk = torch.empty(need // 8, dtype=torch.float64, device="cuda")

        def run():
            _lib.check(L.qn_stack_weights(Lr.data_ptr(), G, K0, 0.0, 10 ** 9, 0, a.iters, w.data_ptr(), status.data_ptr(),
                                          wsk.data_ptr(), need, st), "qn_stack_weights")

        run()
        torch.cuda.synchronize()
        t = float(np.median([window(run, 1) for _ in range(a.windows)])) / a.iters
        emit(what="stack_iter", G=G, K=K0, launches_per_call=a.iters, iter_s=t, bound_s=G * K0 * 8 / HBM,
             done=float(status[-1].item()))

    # ---- qn_pred_score_w beside qn_pred_score
    M = 256
    F, y = data(M, K0, 2)
    wm = torch.full((M,), 1.0 / M, dtype=torch.float64, device="cuda")
    for name, what in (("all rows (pair pass)", 31), ("without the pair pass", 31 & ~_lib.SCORE_CRPS)):
        need = int(L.qn_pred_score_workspace_bytes(M, K0, what))
        wsk = torch.empty(need // 8, dtype=torch.float64, device="cuda")
        t_w, t_p = alternate(
            lambda: _lib.check(L.qn_pred_score_w(F.data_ptr(), None, _lib.QN_F64, y.data_ptr(), wm.data_ptr(), M, K0, 0.7, what,
                                                 out.data_ptr(), wsk.data_ptr(), need, st), "qn_pred_score_w"),
            lambda: _lib.check(L.qn_pred_score(F.data_ptr(), None, _lib.QN_F64, y.data_ptr(), M, K0, 0.7, what, out.data_ptr(),
                                               wsk.data_ptr(), need, st), "qn_pred_score"), a.reps, a.windows)
        emit(what="score_w", rows=name, M=M, K=K0, pred_score_w_s=t_w, pred_score_s=t_p, ratio=t_w / t_p)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
