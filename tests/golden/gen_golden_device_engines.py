#!/usr/bin/env python3
"""Record tests/golden/g17_device_engines.npz (needs the GPU): for every case of tests/test_gpu_device_engine_golden.py the
arrays its `run_case` returns, stored as '<case>.<key>'.  The committed file was written by the engines as they stood BEFORE
they were put on quinn_amd/mcmc/device_engine.py, twice in separate processes with identical results; run it again only when
a chain is changed on purpose:  python tests/golden/gen_golden_device_engines.py [output.npz]
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(HERE, "..", ".."), os.path.join(HERE, "..")]

from test_gpu_device_engine_golden import CASES, GOLDEN, run_case      # noqa: E402

if __name__ == "__main__":
    rec = {f"{name}.{k}": v for name in CASES for k, v in run_case(name).items()}
    np.savez_compressed(sys.argv[1] if len(sys.argv) > 1 else GOLDEN, **rec)
    print({name: float(rec[name + '.accrate'].mean()) for name in CASES})
