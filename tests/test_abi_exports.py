"""CPU: the C-ABI library builds for gfx950, loads, and exports every symbol the header
declares; descriptor / size queries work without a GPU; the product path refuses to run
without one (no CPU fallback)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from quinn_amd import _lib
from quinn_amd.ops import MLPArch, RNetArch, BatchedMLP, kron_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    _lib.build()
    return _lib.lib()


def test_header_symbols_all_exported(L):
    hdr = open(os.path.join(ROOT, "include", "quinn_amd.h")).read()
    declared = set(re.findall(r"\b(qn_[a-z_0-9]+)\s*\(", hdr))
    assert declared == set(_lib.SYMBOLS)
    for s in declared:
        assert hasattr(L, s), s
    assert b"gfx950" in L.qn_version()


vp, i32, i64, u64, f64, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_uint64, ctypes.c_double, ctypes.c_size_t

MINI_HEADER = """
/* a block comment that names qn_in_a_comment(int) and
 * runs over two lines */
#ifndef MINI_H
#define MINI_H
#include <stdint.h>
enum { QN_ONE = 1, QN_MINUS = -2 };   // a line comment with qn_also_ignored(
#define QN_MASK   0x10
#define QN_NOT_A_NUMBER QN_ONE
typedef struct qn_desc qn_desc;
int qn_all_types(const qn_desc* desc, qn_desc** out, int a, int32_t b, int64_t c, uint64_t d, double e, size_t f,
                 const unsigned char* g /* [n] */,
                 const int* h, int64_t *k, void* stream);
int64_t qn_count(const qn_desc* desc);
size_t qn_bytes(int n);
int qn_nothing(void);
const char* qn_text(void);
#endif
"""


def test_parser_on_literal_prototypes():
    functions, constants = _lib.parse_header(MINI_HEADER)
    assert list(functions.items()) == [
        ("qn_all_types", (i32, [vp, vp, i32, i32, i64, u64, f64, sz, vp, vp, vp, vp])),
        ("qn_count", (i64, [vp])),
        ("qn_bytes", (sz, [i32])),
        ("qn_nothing", (i32, [])),
        ("qn_text", (ctypes.c_char_p, []))]
    assert constants == {"QN_ONE": 1, "QN_MINUS": -2, "QN_MASK": 16}


@pytest.mark.parametrize("decl, names", [
    ("int qn_bad(float x);", ("qn_bad", "float x")),                         # a type outside the ABI's vocabulary
    ("int qn_bad(qn_desc desc, int n);", ("qn_bad", "qn_desc desc")),        # a struct by value
    ("int qn_bad(const double* x, int);", ("qn_bad", "int")),                # an unnamed parameter
    ("int qn_bad(const double*, int n);", ("qn_bad", "const double*")),
    ("float qn_bad(int n);", ("qn_bad", "float")),                           # an unknown return type
    ("int qn_bad(int (*callback)(int), int n);", ("qn_bad",)),               # a declaration of another shape
    ("int qn_bad(int n) { return n; }", ("qn_bad",)),
])
def test_parser_is_strict(decl, names):
    with pytest.raises(_lib.QuinnAmdError) as err:
        _lib.parse_header("int qn_good(int n);\n" + decl + "\n")
    for name in names:
        assert name in str(err.value)


# full signatures of the entry points with the longest / most mixed argument lists, copied ONCE from include/quinn_amd.h: the
# only hand copy, here to catch a regression of the parser (not to mirror the ABI)
SPOT = {
    "qn_mcmc_accept_propose": (i32, [vp, vp, f64, i32, i32, i32, i64, i32, u64] + [vp] * 14 +
                               [i32, i64, vp, i32, vp, f64, vp, i32, f64, vp, i32, i32, vp]),
    "qn_sg_step": (i32, [vp, vp, vp, i32, vp, f64, i32, i32, f64, f64, f64, i32, i64, f64, i32, i32, i32, i32, i64, i32, u64] +
                   [vp] * 7 + [i32, vp]),
    "qn_pt_swap": (i32, [vp] * 12 + [i32, i32, i32, i32, i32, i64, i32, u64, i32, i32, vp]),
    "qn_hmc_adapt": (i32, [vp, vp, i32, vp, i32, i32, i64, i32, f64, i32, i32, i32, i32] + [vp] * 6),
    "qn_mlp_sse_fwdbwd": (i32, [vp, i32, vp, vp, vp, vp, i32, i32, i32, vp, vp, vp, vp, sz, vp]),
    "qn_kron_layout": (i32, [vp] * 6),
    "qn_rnet_desc_create": (i32, [i32] * 5 + [vp] + [i32] * 5 + [vp]),
}


def test_real_header(L):
    hdr = open(os.path.join(ROOT, "include", "quinn_amd.h")).read()
    functions, constants = _lib.parse_header(hdr)
    assert len(functions) == len(set(re.findall(r"\b(qn_[a-z_0-9]+)\s*\(", hdr)))
    assert functions == _lib.FUNCTIONS and list(functions) == _lib.SYMBOLS
    for name, (restype, argtypes) in functions.items():
        fn = getattr(L, name)                                    # exported by the built library
        assert (fn.restype, list(fn.argtypes)) == (restype, argtypes), name
    for name, sig in SPOT.items():
        assert functions[name] == sig, name
    assert len(SPOT["qn_mcmc_accept_propose"][1]) == 36 and len(SPOT["qn_sg_step"][1]) == 30


def test_constants_are_the_headers():
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "quinn_amd.h")).read(), flags=re.S)

    def header_value(name):                                      # `#define NAME v` or the enum member `NAME = v`
        (v,) = set(re.findall(r"\b%s\b\s*=?\s*(-?\d+)\b" % name, hdr))
        return int(v)

    public = ["QN_F64", "QN_F32",
              "PATH_AUTO", "PATH_GENERIC", "PATH_FUSED", "PATH_FUSED_DP",
              "ARITH_PLAIN", "ARITH_I8_FUSED", "ARITH_I8_WIDE", "ARITH_I8_LAYERS",
              "CURV_HESS_FULL", "CURV_EF_DIAG", "CURV_GGN_FULL", "CURV_GGN_DIAG",
              "GLM_COV_FULL", "GLM_COV_DIAG",
              "SWAG_INIT", "SWAG_SGD", "SWAG_SGD_COLLECT",
              "SCORE_LPPD", "SCORE_PWAIC", "SCORE_PIT", "SCORE_CRPS", "SCORE_MOMENTS", "SCORE_NOUT"]
    for name in public:
        assert getattr(_lib, name) == header_value(name if name.startswith("QN_") else "QN_" + name), name
    assert _lib.ACT_CODES == {"identity": header_value("QN_ACT_IDENTITY"), "tanh": header_value("QN_ACT_TANH"),
                              "relu": header_value("QN_ACT_RELU")}
    for name in ("QN_OK", "QN_EINVAL", "QN_EWORKSPACE", "QN_EHIP", "QN_EUNSUPPORTED"):
        assert _lib.CONSTANTS[name] == header_value(name), name
    assert _lib.CONSTANTS["QN_OK"] == 0 and _lib.CONSTANTS["QN_EINVAL"] == -1


def test_kron_layout_through_void_pointers(L):
    """int64 arrays and byref() scalars through the c_void_p parameters of qn_kron_layout."""
    arch = MLPArch((3, 5, 4, 2), "tanh")
    dims = (ctypes.c_int * 4)(*arch.dims)
    h = ctypes.c_void_p()
    assert L.qn_mlp_desc_create(dims, 4, _lib.ACT_CODES["tanh"], 1, ctypes.byref(h)) == 0
    oa, os_, ok = ((ctypes.c_int64 * 3)() for _ in range(3))
    la, ls = ctypes.c_int64(), ctypes.c_int64()
    assert L.qn_kron_layout(h, oa, os_, ok, ctypes.byref(la), ctypes.byref(ls)) == 0
    assert L.qn_kron_layout(h, None, None, None, None, None) == 0          # any pointer may be NULL
    assert L.qn_mlp_desc_destroy(h) == 0
    lay = kron_layout(arch, L)
    assert (tuple(oa), tuple(os_), tuple(ok), la.value, ls.value) == (lay.offA, lay.offS, lay.offK, lay.lenA, lay.lenS)
    assert lay.offA == (0, 16, 52) and lay.lenA == 16 + 36 + 25 and lay.offS == (0, 25, 41) and lay.lenS == 25 + 16 + 4
    assert lay.offK == (0, 20, 44) and lay.p == arch.nparams == 54


def test_rnet_descriptor_through_void_pointers(L):
    """A double array and an unsigned-char array through the c_void_p parameters of the residual-net descriptor calls."""
    arch = RNetArch(3, 3, 3, 2, ((1.0, 0.0), (1.0, 0.5)), "tanh", uses=((True, False), (True, True)))
    coef = (ctypes.c_double * 4)(1.0, 0.0, 1.0, 0.5)
    h = ctypes.c_void_p()
    assert L.qn_rnet_desc_create(3, 3, 3, 2, 2, coef, _lib.ACT_CODES["tanh"], 1, 0, 0, 0, ctypes.byref(h)) == 0
    assert L.qn_rnet_desc_set_uses(h, (ctypes.c_ubyte * 4)(1, 0, 1, 1), 4) == 0
    assert L.qn_rnet_desc_set_uses(h, (ctypes.c_ubyte * 3)(1, 0, 1), 3) == -1          # n must be nsteps * npar
    assert L.qn_mlp_num_params(h) == arch.nparams == 2 * 9 + 2 * 3
    assert L.qn_mlp_desc_destroy(h) == 0
    h2 = arch.create_desc(L)
    assert L.qn_mlp_num_params(h2) == 24
    assert L.qn_mlp_desc_destroy(h2) == 0


def test_descriptor_and_sizes(L):
    dims = (ctypes.c_int * 5)(1, 64, 64, 64, 1)
    h = ctypes.c_void_p()
    assert L.qn_mlp_desc_create(dims, 5, 1, 1, ctypes.byref(h)) == 0
    assert L.qn_mlp_num_params(h) == 8513 == MLPArch((1, 64, 64, 64, 1)).nparams
    assert L.qn_workspace_bytes(h, 64, 4096, 1, 0) > 0
    assert L.qn_mlp_path(h, 64, 4096, 0, 0) in (_lib.PATH_GENERIC, _lib.PATH_FUSED)
    assert L.qn_mlp_desc_destroy(h) == 0
    bad = (ctypes.c_int * 2)(3, 0)
    assert L.qn_mlp_desc_create(bad, 2, 1, 1, ctypes.byref(h)) == -1
    assert b"dims" in L.qn_last_error()
    assert L.qn_mlp_desc_create(dims, 5, 7, 1, ctypes.byref(h)) == -1


def test_arch_extraction():
    seq = torch.nn.Sequential(torch.nn.Linear(2, 5), torch.nn.Tanh(), torch.nn.Linear(5, 1))
    a = MLPArch.from_module(seq)
    assert a.dims == (2, 5, 1) and a.activ == "tanh" and a.bias and a.nparams == 21   # numpar()==21
    from quinn_amd.nns.mlp import MLP
    m = MLP(1, 1, (16, 16), activ='tanh')
    assert MLPArch.from_module(m).dims == (1, 16, 16, 1) and m.numpar() == 321
    with pytest.raises(NotImplementedError):
        MLPArch.from_module(torch.nn.Sequential(torch.nn.Linear(2, 2), torch.nn.Sigmoid(), torch.nn.Linear(2, 1)))
    with pytest.raises(NotImplementedError):
        MLPArch.from_module(torch.nn.Conv1d(1, 1, 1))


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU failure mode")
def test_no_cpu_fallback():
    with pytest.raises(_lib.QuinnAmdError):
        BatchedMLP(MLPArch((1, 4, 1)), np.zeros((3, 1)), np.zeros((3, 1)))
