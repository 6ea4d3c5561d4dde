"""GPU, runs FIRST (file name): the multi-rank paths as child programs, started before this pytest process has touched
the GPU (a GPU-initialised process must not start child programs on these boxes).  On a 1-GPU box the ranks share
cuda:0 and use gloo for the collectives; what is checked is the launch / shard / gather logic:
  * `bench.py --gpus 2` starts its own two ranks and prints ONE JSON line with n_gpus = 2, weak and strong scaling;
  * a plain `bench.py` run times ONE region of exactly --steps steps and `--dump-outputs` writes what its last step returned;
  * `NN_MCMC.fit(engine='device')` under two ranks equals the single-process run for AMCMC and for HMC (random streams
    keyed by the global chain id), with gather = 'all' and gather = 'root'."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from quinn_amd.parallel import launch_ranks

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _no_gpu_yet():
    if torch.cuda.is_initialized():
        pytest.skip("this process has already initialised the GPU: child programs are not started from it")


def _json_lines(text):
    """Every top-level JSON object in `text` (two ranks may print onto one line)."""
    dec, out, i = json.JSONDecoder(), [], text.find("{")
    while i >= 0:
        try:
            obj, end = dec.raw_decode(text, i)
            out.append(obj)
            i = text.find("{", end)
        except json.JSONDecodeError:
            i = text.find("{", i + 1)
    return out


@pytest.mark.parametrize("scaling", ["weak", "strong"])
def test_bench_gpus_2_starts_two_ranks(scaling, tmp_path):
    _no_gpu_yet()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--scaling", scaling, "--steps", "20",
                        "--warmup", "2", "--regions", "3", "--full", "--dump-outputs", str(tmp_path)],
                       capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = _json_lines(r.stdout)
    assert len(lines) == 1
    d = lines[0]
    assert d["n_gpus"] == 2 and d["scaling"] == scaling and d["steps"] == 20
    assert d["config"]["chains_total"] == (128 if scaling == "weak" else 64)
    assert d["config"]["chains_rank0"] == (64 if scaling == "weak" else 32)
    assert d["value"] > 0 and d["roofline"]["kernel_ms_min"] <= d["roofline"]["kernel_ms_median"] <= d["roofline"]["kernel_ms_max"]
    assert abs(d["value"] - d["config"]["chains_total"] * 20 / (d["ms_per_step"] * 20e-3)) <= 1e-6 * d["value"]
    assert d["config"]["timed_regions"] == 3 and len(d["config"]["region_ms_per_step"]) == 3
    sse = np.load(tmp_path / "sse.npy")                               # every chain of the job, gathered on rank 0
    assert sse.shape == (d["config"]["chains_total"],) and np.isfinite(sse).all() and (sse > 0).all()


def test_bench_plain_run_times_the_steps_once_and_dumps_the_last_step(tmp_path):
    """A plain run (no --full): ONE timed region of exactly --steps steps, the headline fields and nothing that takes runs of
    its own.  --dump-outputs writes what the last timed step returned (here: SSE and gradient of all 64 chains), which must be
    the oracle's values for that step's weights (step 19 of a 10-step graph replayed twice: resident weight batch 9 % 8 = 1)."""
    _no_gpu_yet()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "20", "--warmup", "2", "--graph", "10",
                        "--kind", "grad", "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = _json_lines(r.stdout)
    assert len(lines) == 1
    d = lines[0]
    assert all(k in d for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"))
    assert d["steps"] == 20 and d["config"]["timed_regions"] == 1 and len(d["config"]["region_ms_per_step"]) == 1
    assert not {"roofline", "extras", "cpu_baseline"} & set(d)
    assert abs(d["value"] - 64 * 20 / (d["ms_per_step"] * 20e-3)) <= 1e-6 * d["value"]
    sse, grad = np.load(tmp_path / "sse.npy"), np.load(tmp_path / "grad.npy")
    assert sse.shape == (64,) and sse.dtype == np.float64 and grad.shape == (64, 8513) and grad.dtype == np.float64
    import bench
    from oracle import mlp_ref
    from quinn_amd.ops import neg_log_post_from_sse
    x, y = bench.synthetic(bench.N, bench.DIMS[0])
    mod = mlp_ref.build_module(mlp_ref.MLPSpec(bench.DIMS, "tanh"))
    yd = [v for v in y]
    for c in (0, 37, 63):
        W = 0.1 * np.random.RandomState(1000 + c + 100003 * 1).randn(8513)
        ref = mlp_ref.logpost(mod, W, x, yd, bench.SIGMA)
        got = -neg_log_post_from_sse(sse[c], bench.N, bench.SIGMA)
        assert abs(got - ref) <= 1e-11 * abs(ref), (c, got, ref)
        gref = mlp_ref.logpostgrad(mod, W, x, yd, bench.SIGMA)
        assert np.max(np.abs(-(0.5 * grad[c] / bench.SIGMA ** 2) - gref)) <= 1e-9 * np.max(np.abs(gref)), c


def test_bench_one_rank_with_a_live_rccl_process_group_prints_one_json_line():
    """QN_BENCH_FORCE_DIST=1: one rank creates the RCCL process group (communicator on cuda:0, the probe all_reduce, the barriers of
    every timed region, the closing all_gather, graph capture beside the live group) -- everything of the driver's N > 1 launch but
    the transport between ranks.  RCCL prints a version banner on stdout while the communicator is made: bench.py points fd 1 at
    stderr for that time, so that stdout is exactly the one JSON line the driver parses."""
    _no_gpu_yet()
    from quinn_amd.parallel import free_port
    env = dict(os.environ, QN_BENCH_FORCE_DIST="1", WORLD_SIZE="1", RANK="0", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1",
               MASTER_PORT=str(free_port()), HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("QN_BENCH_BACKEND", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "20", "--warmup", "2", "--regions", "3", "--no-extras",
                        "--no-cpu-baseline"], capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    out = r.stdout.strip()
    assert out.count("\n") == 0 and out.startswith("{") and out.endswith("}"), out[:400]
    d = json.loads(out)
    assert d["n_gpus"] == 1 and d["value"] > 0 and "nccl process group" in d["config"]["rehearsal"]


def test_gather_rows_through_rccl_with_one_rank():
    """`quinn_amd.parallel.gather_rows` / `gather_results` on device tensors through RCCL's all_gather_into_tensor / gather (one
    rank, QN_FORCE_GATHER=1): piece loop, every dtype the result dicts carry, root / all modes (tests/rccl_one_rank_worker.py)."""
    _no_gpu_yet()
    from quinn_amd.parallel import free_port
    env = dict(os.environ, QN_FORCE_GATHER="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(free_port()), HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "rccl_one_rank_worker.py")], capture_output=True, text=True,
                       timeout=600, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stdout.strip().splitlines()[-1] == "rccl one-rank gather ok", r.stdout[-500:]      # (MLP prints its parameter count, as the reference does)


def test_bench_rank_without_a_gpu_of_its_own_exits_with_one_clear_line():
    """Two RCCL ranks on a one-GPU box (launched as the driver launches them, no gloo rehearsal): the rank that has no GPU says
    so in one line and exits non-zero, torchrun ends the other one and returns a non-zero code; nothing hangs or restarts."""
    _no_gpu_yet()
    import torch
    if torch.cuda.device_count() != 1:
        pytest.skip("needs a box with exactly one GPU")
    from quinn_amd.parallel import free_port
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("QN_BENCH_BACKEND", None)
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", str(free_port()), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "4", "--warmup", "1"],
                       capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert r.returncode != 0
    lines = [ln for ln in r.stderr.splitlines() if ln.startswith("bench.py: rank")]
    assert len(lines) >= 1 and "GPU(s) visible" in lines[0], r.stderr[-2000:]
    assert not _json_lines(r.stdout)


@pytest.mark.parametrize("sampler,gather", [("amcmc", "all"), ("hmc", "all"), ("hmc", "root")])
def test_device_engine_two_ranks_equal_one_process(sampler, gather):
    _no_gpu_yet()
    tool = os.path.join(ROOT, "tools", "check_device_2rank.py")
    one = subprocess.run([sys.executable, tool, sampler, gather], capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert one.returncode == 0, one.stderr[-3000:]
    ref = _json_lines(one.stdout)[-1]
    rc, so, se = launch_ranks(tool, [sampler, gather], 2, timeout=900, capture=True)
    assert rc == 0, se[-3000:]
    outs = {d["rank"]: d for d in _json_lines(so)}
    assert set(outs) == {0, 1}
    keys = ("accrate", "maxpost", "last_logpost", "chain_checksum")
    assert outs[0]["chains"] == ref["chains"]                         # rank 0 holds every chain under 'all' and 'root'
    for k in keys:
        assert outs[0][k] == pytest.approx(ref[k], rel=1e-6, abs=1e-4), k
    if gather == "all":
        assert all(outs[1][k] == outs[0][k] for k in keys)
    else:                                                             # rank 1 keeps its own shard (chains 3..5)
        assert outs[1]["chains"][0] == 3
        for k in keys:
            assert outs[1][k] == pytest.approx(ref[k][3:], rel=1e-6, abs=1e-4), k


@pytest.mark.parametrize("kind", ["ens", "rms"])
def test_ensemble_members_shard_over_two_ranks(kind):
    """NN_Ens / NN_RMS: members block-partitioned over the ranks, one all_gather -- every rank ends up with every member's
    weights, histories and predictions, equal to the single-process run."""
    _no_gpu_yet()
    tool = os.path.join(ROOT, "tools", "check_ens_2rank.py")
    one = subprocess.run([sys.executable, tool, kind], capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert one.returncode == 0, one.stderr[-3000:]
    ref = _json_lines(one.stdout)[-1]
    rc, so, se = launch_ranks(tool, [kind], 2, timeout=900, capture=True)
    assert rc == 0, se[-3000:]
    outs = {d["rank"]: d for d in _json_lines(so)}
    assert set(outs) == {0, 1}
    for r in (0, 1):
        assert outs[r]["members"] == ref["members"] == 5
        for k in ("best_w_checksum", "final_w_checksum", "best_loss", "pred_checksum"):
            assert outs[r][k] == pytest.approx(ref[k], rel=1e-7, abs=1e-7), (r, k)
