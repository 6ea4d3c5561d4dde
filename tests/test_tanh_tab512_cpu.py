"""CPU: qn_tanh_f64_tab512 (csrc/qn_tanh512.h, the activation of the 8-wave int8-slice forward) compiled into a small host
program -- the header is free of device-only calls for exactly this -- against an extended-precision reference
(mpmath at 200 bits, Python's decimal at 50 digits without it): every table node n / 512, every midpoint between two nodes
(the largest |b| of the range reduction) and 10^5 random points in [-21, 21].  Absolute error < 2^-51 everywhere."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "quinn_amd", "csrc")

PROGRAM = r"""
#include "qn_tanh512.h"
#include <cstdio>
#include <vector>
static const double tab[QN_TANH_TAB512_N] = {QN_TANH_TAB512_VALUES};
int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 3;
    std::vector<double> x;
    double v;
    while (std::fread(&v, 8, 1, f) == 1) x.push_back(v);
    std::fclose(f);
    for (double& e : x) e = qn_tanh_f64_tab512(e, tab);
    f = std::fopen(argv[2], "wb");
    if (!f) return 4;
    std::fwrite(x.data(), 8, x.size(), f);
    std::fclose(f);
    return 0;
}
"""


def _reference(x):
    """tanh(x) - float(tanh(x)) is what matters below: return the reference as (nearest double, remainder) pairs."""
    try:
        import mpmath
        mpmath.mp.prec = 200
        ref = [mpmath.tanh(mpmath.mpf(float(v))) for v in x]
        hi = np.array([float(r) for r in ref])
        lo = np.array([float(r - mpmath.mpf(float(h))) for r, h in zip(ref, hi)])
        return hi, lo
    except ImportError:
        from decimal import Decimal, getcontext
        getcontext().prec = 50
        hi, lo = [], []
        for v in x:
            d = Decimal(float(v))
            e = (-2 * abs(d)).exp()
            r = (1 - e) / (1 + e)
            r = -r if d < 0 else r
            h = float(r)
            hi.append(h)
            lo.append(float(r - Decimal(h)))
        return np.array(hi), np.array(lo)


@pytest.fixture(scope="module")
def tanh512(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler to build the tanh(n / 512) check with")
    d = tmp_path_factory.mktemp("tanh512")
    src, exe = d / "t512.cpp", d / "t512"
    src.write_text(PROGRAM)
    # (-ffp-contract=off: the host arithmetic is the header's fma calls and nothing else, as on the device)
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-I", CSRC, str(src), "-o", str(exe)], check=True)

    def run(x):
        xin, xout = d / "in.bin", d / "out.bin"
        np.asarray(x, dtype=np.float64).tofile(xin)
        subprocess.run([str(exe), str(xin), str(xout)], check=True)
        return np.fromfile(xout, dtype=np.float64)
    return run


def _check(run, x):
    got = run(x)
    hi, lo = _reference(x)
    err = np.abs((got - hi) - lo)                      # got - hi is exact (neighbouring doubles), lo is tiny
    k = int(np.argmax(err))
    print(f"{len(x)} points: max |error| = 2^{np.log2(max(err[k], 1e-300)):.2f} at x = {x[k]!r}")
    assert err[k] < 2.0 ** -51, (x[k], got[k], hi[k], err[k])


def test_nodes(tanh512):
    n = np.arange(10241, dtype=np.float64)
    _check(tanh512, np.concatenate([n / 512, -n / 512]))


def test_midpoints(tanh512):
    n = np.arange(10240, dtype=np.float64)
    m = (n + 0.5) / 512
    # the midpoint itself (a tie of the rounding to a node) and its two neighbours, which round to different nodes
    _check(tanh512, np.concatenate([m, np.nextafter(m, 0.0), np.nextafter(m, 100.0), -m]))


def test_random_points(tanh512):
    rs = np.random.RandomState(512)
    x = np.concatenate([rs.uniform(-21.0, 21.0, size=100000 - 8), [0.0, -0.0, 20.0, -20.0, 21.0, -21.0, 1e-300, -1e-9]])
    _check(tanh512, x)
    # odd, and the clamp: beyond 20 the result is the table's last node
    got = tanh512(np.array([3.7, -3.7, 25.0, 1e300, -np.inf]))
    assert got[0] == -got[1] and got[2] == got[3] == -got[4] == 1.0
