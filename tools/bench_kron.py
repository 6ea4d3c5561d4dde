#!/usr/bin/env python3
"""Kronecker-factored Laplace kernels (qn_kron.hip) on the MI355X, float64 tanh networks:

    cfg2  64 members of (1,64,64,64,1),         N = 4096
    cfg3  128 members of (1,128,128,128,1),     N = 8192
    cfg4  64 members of (1,256,256,256,256,1),  N = 16384

    python tools/bench_kron.py [--cfg cfg2 cfg3 cfg4] [--reps 3] [--no-torch] [--stats-csv FILE] [--counters-csv FILE]
                               [--out profiles/kron_laplace.txt]

Per shape: whole-call time of `kron_factors`, of `kron_glm_predict` at 4096 query rows and of `kron_sample` for 100 draws (the
sampler call is repeated inside the timed window until it has run for about a quarter of a second), the algorithmic flop counts
of DESIGN 4.4 over those WHOLE-CALL times against the 78.6 TFLOP/s float64 MFMA peak (whole-call rates: launches, the row pass
and the reduce are in the time; they are not a kernel's share of peak), and two comparisons on the same card:
(a) `curvature(W, 'ggn_diag')` at the same shape, (b) torch forming the same factors by `bmm` from activations it computed itself.

The split of `kron_factors` into the row pass (k_jac_rows) and the factor products (k_kron_syrk + k_kron_reduce), and the HBM
bytes, come from two profiler runs of their own, each of this script with `--no-torch --reps 1 --out ''`:
    rocprofv3 --kernel-trace --stats -d DIR -o trace -- python tools/bench_kron.py --cfg cfg4 --no-torch --reps 1 --out ''
    rocprofv3 --pmc FETCH_SIZE WRITE_SIZE -d DIR -o pmc -- python tools/bench_kron.py --cfg cfg4 --no-torch --reps 1 --out ''
(counters alone in the second run, no tracing beside them).  A later plain run given `--stats-csv DIR/.../trace_kernel_stats.csv`
and `--counters-csv DIR/.../pmc_counter_collection.csv` adds the per-kernel seconds and the per-kernel HBM bytes (FETCH_SIZE and
WRITE_SIZE are in KiB) to the file.  One warm-up call, then the median of the reps."""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from quinn_amd.ops import MLPArch, BatchedMLP, kron_sample    # noqa: E402

PEAK_F64 = 78.6e12
CFGS = {"cfg2": (64, (1, 64, 64, 64, 1), 4096), "cfg3": (128, (1, 128, 128, 128, 1), 8192),
        "cfg4": (64, (1, 256, 256, 256, 256, 1), 16384)}
NQ, DRAWS = 4096, 100
KERNELS = ("k_jac_rows", "k_kron_syrk", "k_kron_reduce", "k_kron_rotate", "k_kron_glm", "k_kron_sample")


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


def flop_counts(arch, B, N, nq, draws):
    """Algorithmic flops: factors = one triangle of every rank-N update; glm = rotations + T product + contraction;
    sample = the two rotations of every layer block."""
    o = arch.dims[-1]
    e = [d + 1 for d in arch.dims[:-1]]
    h = list(arch.dims[1:])
    factors = B * N * sum(ei * (ei + 1) + o * hi * (hi + 1) for ei, hi in zip(e, h))
    glm = B * nq * sum(2 * ei * ei + 2 * o * hi * hi + 2 * ei * hi + 3 * hi * o * (o + 1) // 2 for ei, hi in zip(e, h))
    sample = draws * sum(2 * hi * ei * ei + 2 * hi * hi * ei for ei, hi in zip(e, h))
    return factors, glm, sample


def torch_factors(arch, W, X):
    """The same factors by bmm from activations torch computes itself (tanh MLP with biases), all members at once."""
    B, N = W.shape[0], X.shape[0]
    L = len(arch.dims) - 1
    o = arch.dims[-1]
    Ws, bs, off = [], [], 0
    for a, b in zip(arch.dims[:-1], arch.dims[1:]):
        Ws.append(W[:, off:off + a * b].view(B, b, a)); off += a * b
        bs.append(W[:, off:off + b]); off += b
    one = torch.ones(B, N, 1, dtype=W.dtype, device=W.device)
    ins, h = [], X.unsqueeze(0).expand(B, N, -1)
    for i in range(L):
        ins.append(torch.cat([h, one], dim=2))
        z = torch.baddbmm(bs[i].unsqueeze(1), h, Ws[i].transpose(1, 2))
        h = torch.tanh(z) if i + 1 < L else z
    A = [t.transpose(1, 2) @ t for t in ins]
    S = [None] * L
    for k in range(o):
        g = torch.zeros(B, N, o, dtype=W.dtype, device=W.device)
        g[:, :, k] = 1.0
        for i in range(L - 1, -1, -1):
            s = g.transpose(1, 2) @ g
            S[i] = s if S[i] is None else S[i] + s
            if i > 0:
                a = ins[i][:, :, :-1]
                g = (g @ Ws[i]) * (1.0 - a * a)
    return A, S


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cfg", nargs="+", default=list(CFGS))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--stats-csv", default=None)
    ap.add_argument("--counters-csv", default=None)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "kron_laplace.txt"), help="'' writes no file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_kron.py needs the MI355X"
    lines = []
    for name in a.cfg:
        B, dims, N = CFGS[name]
        arch = MLPArch(dims, "tanh")
        p = arch.nparams
        rs = np.random.RandomState(0)
        x = rs.rand(N, 1) * 2 - 1
        op = BatchedMLP(arch, x, None, device="cuda:0")
        Wd = op.weights(rs.randn(B, p) / np.sqrt(max(dims)))
        t_f, ts_f = gpu_time(lambda: op.kron_factors(Wd), a.reps)
        A, S, lay = op.kron_factors(Wd)
        UA, US = torch.empty_like(A), torch.empty_like(S)
        Dinv = torch.empty(B, p, dtype=torch.float64, device="cuda:0")
        for i in range(len(lay.e)):
            la_, ua = torch.linalg.eigh(lay.A(A, i))
            ls_, us = torch.linalg.eigh(lay.S(S, i))
            lay.A(UA, i).copy_(ua), lay.S(US, i).copy_(us)
            lay.K(Dinv, i).copy_(1.0 / (ls_.clamp_min(0)[:, :, None] * la_.clamp_min(0)[:, None, :] / (N * 0.01) + 1.0))
        xq = rs.rand(NQ, 1) * 2 - 1
        t_g, ts_g = gpu_time(lambda: op.kron_glm_predict(Wd, UA, US, Dinv, xq), a.reps)
        js = rs.randint(0, B, DRAWS)
        Z = torch.randn(DRAWS, p, dtype=torch.float64, device="cuda:0")
        Dih = Dinv.sqrt()
        one = lambda: kron_sample(arch, Wd, UA, US, Dih, js, Z, op=op)        # noqa: E731
        t1, _ = gpu_time(one, 1)
        loops = max(1, int(np.ceil(0.25 / max(t1, 1e-6))))                     # time enough work: ~0.25 s per timed window
        t_s, ts_s = gpu_time(lambda: [one() for _ in range(loops)], a.reps)
        t_s, ts_s = t_s / loops, [t / loops for t in ts_s]
        t_d, ts_d = gpu_time(lambda: op.curvature(Wd, "ggn_diag"), a.reps)
        ff, fg, fs = flop_counts(arch, B, N, NQ, DRAWS)
        rec = dict(what="kron", cfg=name, shape="%d x %s tanh, N=%d, p=%d" % (B, dims, N, p),
                   factors_s=t_f, factors_runs_s=ts_f, factors_flop=ff, factors_whole_call_tflops=ff / t_f / 1e12,
                   factors_whole_call_frac_of_f64_mfma_peak=ff / t_f / PEAK_F64,
                   glm_s=t_g, glm_runs_s=ts_g, glm_query_rows=NQ, glm_flop=fg, glm_whole_call_tflops=fg / t_g / 1e12,
                   glm_whole_call_frac_of_f64_mfma_peak=fg / t_g / PEAK_F64,
                   sample_s=t_s, sample_runs_s=ts_s, sample_draws=DRAWS, sample_calls_per_window=loops, sample_flop=fs,
                   sample_whole_call_tflops=fs / t_s / 1e12,
                   ggn_diag_s=t_d, ggn_diag_runs_s=ts_d, factors_over_ggn_diag=t_f / t_d)
        if not a.no_torch:
            t_t, ts_t = gpu_time(lambda: torch_factors(arch, Wd, op.X), a.reps)
            At, St = torch_factors(arch, Wd, op.X)
            diff = max(float((lay.A(A, i) - At[i]).abs().max() / At[i].abs().max()) for i in range(len(lay.e)))
            diff = max(diff, max(float((lay.S(S, i) - St[i]).abs().max() / St[i].abs().max()) for i in range(len(lay.e))))
            rec.update(torch_bmm_s=t_t, torch_bmm_runs_s=ts_t, torch_over_kernel=t_t / t_f, max_rel_diff_vs_torch=diff)
        s = json.dumps(rec)
        print(s, flush=True)
        lines.append(s)
    if a.stats_csv:                                           # kernel statistics of a trace run of this script (its own run)
        tot = {}
        with open(a.stats_csv) as fh:
            for row in csv.DictReader(fh):
                nm = row.get("Name", "")
                for key in KERNELS:
                    if key in nm:
                        tot[key] = tot.get(key, 0.0) + float(row.get("TotalDurationNs", 0.0)) * 1e-9
        s = json.dumps(dict(what="kernel totals from the trace (all shapes and reps of that run)", seconds=tot))
        print(s, flush=True)
        lines.append(s)
    if a.counters_csv:                                        # a counters-only run of this script (its own run)
        kib = {}
        with open(a.counters_csv) as fh:
            for row in csv.DictReader(fh):
                nm, cn = row.get("Kernel_Name", ""), row.get("Counter_Name", "")
                for key in KERNELS:
                    if key in nm and cn in ("FETCH_SIZE", "WRITE_SIZE"):
                        d = kib.setdefault(key, {"FETCH_SIZE": 0.0, "WRITE_SIZE": 0.0})
                        d[cn] += float(row.get("Counter_Value", 0.0))
        s = json.dumps(dict(what="HBM bytes per kernel from the counters-only run (all shapes and calls of that run)",
                            bytes={k: {c: v * 1024.0 for c, v in d.items()} for k, d in kib.items()}))
        print(s, flush=True)
        lines.append(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("# tools/bench_kron.py --reps %d --cfg %s\n" % (a.reps, " ".join(a.cfg)))
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
