#!/usr/bin/env python3
"""qn_rank_diag (csrc/qn_rank.hip) on the MI355X, timed alternately with qn_chain_stats on the same chains and burn-in.

    python tools/bench_rank_diag.py [--reps 3] [--windows 5] [--small-only] [--out profiles/rank_diag.txt]

Shapes [C, T, K] float64: the cfg2 parameter chain [64, 2000, 8513], predictions [64, 128, 4096], the log-posterior trace
[64, 2000, 1] and one long chain [1, 16384, 64]; nburn = 0, the plan of `rankdiag.rank_plan` (so the first and third are thinned
to 16384 pooled draws).  Per shape one JSON line: the seconds of both passes (device-event times of `reps` back-to-back calls
after a warm-up call that also settles the clock, the two passes alternating window by window, median over `windows`), the
bytes qn_rank_diag requests (the window read once, written to the workspace and read back eight times as float64, z
written and read twice) against the window's own size.  A last line bounds the share of the time the two sorts take
(`sort_share`)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from quinn_amd import _lib                                       # noqa: E402
from quinn_amd.mcmc import diagnostics as diag                   # noqa: E402
from quinn_amd.mcmc import rankdiag                              # noqa: E402

SHAPES = [(64, 2000, 8513), (64, 128, 4096), (64, 2000, 1), (1, 16384, 64)]


def window_time(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / 1e3 / reps


def bench_shape(shape, reps, windows):
    C, T, K = shape
    x = torch.empty(C, T, K, dtype=torch.float64, device="cuda")
    for c in range(C):
        x[c].normal_()
    L = _lib.lib()
    st = _lib.stream()
    t0, nh, stride = rankdiag.rank_plan(C, T)
    need = L.qn_rank_diag_workspace_bytes(C, T, K, nh, stride)
    ws = torch.empty(need // 8, dtype=torch.float64, device="cuda")
    out = torch.empty(_lib.RANK_NOUT, K, dtype=torch.float64, device="cuda")
    b0, nbatch, blen = diag.batch_plan(T, 0)
    cneed = L.qn_chain_stats_workspace_bytes(C, T, K, nbatch, blen)
    cws = torch.empty(cneed // 8, dtype=torch.float64, device="cuda")
    stats = torch.empty(C, 6, K, dtype=torch.float64, device="cuda")

    def rank():
        _lib.check(L.qn_rank_diag(x.data_ptr(), _lib.QN_F64, C, T, K, t0, nh, stride, out.data_ptr(), ws.data_ptr(), need, st),
                   "qn_rank_diag")

    def classic():
        _lib.check(L.qn_chain_stats(x.data_ptr(), _lib.QN_F64, C, T, K, b0, nbatch, blen, stats.data_ptr(), cws.data_ptr(), cneed,
                                    st), "qn_chain_stats")

    for _ in range(3):                                           # warm-up: the LDS attribute, the clock
        rank()
        classic()
    torch.cuda.synchronize()
    tr, tc = [], []
    for _ in range(windows):                                     # alternately, so a drifting clock hits both alike
        tr.append(window_time(rank, reps))
        tc.append(window_time(classic, reps))
    S = 2 * C * nh
    win = S * K * 8
    requested = win * (1 + 1 + 8 + 2 + 2)                        # gather read + write, eight reads of x, z written and read twice
    return dict(shape=list(shape), t0=t0, nh=nh, stride=stride, n_draws=S, rank_s=float(np.median(tr)), rank_runs_s=tr,
                chain_stats_s=float(np.median(tc)), chain_stats_runs_s=tc, window_bytes=win, requested_bytes=requested,
                requested_over_window=requested / win, workspace_bytes=int(need), finite=bool(torch.isfinite(out).all()))


def sort_share(reps, windows):
    """The share of k_rank_entry's time spent in its two sorts at S = 16384, from two timings of the one kernel: [64, 128, K]
    as it is, and the same call with nh = 4 per half of 2048 chains -- the same S, the same two sorts and rank searches, but
    sequences of 4 draws, whose autocovariance work is a few lags of 4 terms.  The difference is the series work at nh = 128;
    what remains is sort + search + normalisation, reported as an upper bound of the sort's share."""
    K = 512
    L = _lib.lib()
    st = _lib.stream()
    res = {}
    for name, (C, nh) in (("nh128", (64, 128)), ("nh4", (2048, 4))):
        x = torch.randn(C, 2 * nh, K, dtype=torch.float64, device="cuda")
        need = L.qn_rank_diag_workspace_bytes(C, 2 * nh, K, nh, 1)
        ws = torch.empty(need // 8, dtype=torch.float64, device="cuda")
        out = torch.empty(_lib.RANK_NOUT, K, dtype=torch.float64, device="cuda")

        def call():
            _lib.check(L.qn_rank_diag(x.data_ptr(), _lib.QN_F64, C, 2 * nh, K, 0, nh, 1, out.data_ptr(), ws.data_ptr(), need, st),
                       "qn_rank_diag")

        call()
        torch.cuda.synchronize()
        res[name] = float(np.median([window_time(call, reps) for _ in range(windows)]))
    return dict(sort_probe_K=K, nh128_s=res["nh128"], nh4_s=res["nh4"], sort_search_share_upper_bound=res["nh4"] / res["nh128"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--small-only", action="store_true", help="skip the 8.7 GB shape")
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_rank_diag.py measures on the GPU; none is visible")
    lines = [dict(device=torch.cuda.get_device_name(0), reps=a.reps, windows=a.windows)]
    print(json.dumps(lines[0]), flush=True)
    for shape in SHAPES:
        if a.small_only and shape[0] * shape[1] * shape[2] * 8 > (4 << 30):
            continue
        lines.append(bench_shape(shape, a.reps, a.windows))
        print(json.dumps(lines[-1]), flush=True)
        torch.cuda.empty_cache()
    lines.append(sort_share(a.reps, a.windows))
    print(json.dumps(lines[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
