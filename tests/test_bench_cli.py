"""CPU: bench.py's command line and its output dump (nothing here launches a kernel)."""
import sys

import numpy as np

import bench


def test_a_plain_run_is_one_region_without_the_full_measurements(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "3"])
    a = bench.parse_args()
    assert a.steps == 7 and a.warmup == 3 and a.gpus == 1
    assert not a.full and a.regions is None and a.dump_outputs is None
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "out"])
    a = bench.parse_args()
    assert a.full and a.dump_outputs == "out"


def test_dump_outputs_writes_each_array_as_npy(tmp_path):
    arrays = {"sse": np.linspace(1.0, 2.0, 64), "grad": np.arange(64 * 5, dtype=np.float32).reshape(64, 5)}
    bench.dump_outputs(str(tmp_path / "d"), arrays)
    for name, a in arrays.items():
        got = np.load(tmp_path / "d" / f"{name}.npy")
        assert got.dtype == a.dtype and np.array_equal(got, a)


def test_dump_outputs_keeps_a_fixed_subset_of_rows_within_the_limit(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 1 << 20)
    big = np.random.RandomState(0).randn(300, 1000)                    # 2.4 MB against a 1 MiB limit
    bench.dump_outputs(str(tmp_path), {"grad": big})
    got = np.load(tmp_path / "grad.npy")
    assert got.nbytes <= 1 << 20 and got.shape[1] == 1000 and got.shape[0] > 100
    assert np.array_equal(got[0], big[0]) and np.array_equal(got[-1], big[-1])
    bench.dump_outputs(str(tmp_path / "again"), {"grad": big})
    assert np.array_equal(np.load(tmp_path / "again" / "grad.npy"), got)
