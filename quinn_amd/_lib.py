"""ctypes binding of the C-ABI library (include/quinn_amd.h) and its in-tree build.

The product path has no CPU fallback: if libquinn_amd.so is missing or a call fails,
an exception is raised.
"""
import ctypes
import os
import re
import subprocess

# torch ships its own HIP runtime (torch/lib/libamdhip64.so, same SONAME as /opt/rocm's).
# It must be the one already mapped when this library is loaded, otherwise the process ends
# up with two runtimes and ours sees no device / cannot share torch's streams and memory.
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
LIBDIR = os.path.join(_HERE, "lib")
LIBPATH = os.path.join(LIBDIR, "libquinn_amd.so")
SOURCES = ["qn_api.hip", "qn_generic.hip", "qn_fused.hip", "qn_fused_d8.hip", "qn_fused_o16.hip", "qn_fused_i8.hip", "qn_fused_bwd_i8.hip", "qn_wide_i8.hip", "qn_wide_u_i8.hip", "qn_dw_i8.hip", "qn_mcmc.hip", "qn_hmc_leap.hip", "qn_hmc_adapt.hip", "qn_temper.hip", "qn_sgmcmc.hip", "qn_prior.hip", "qn_hyper.hip", "qn_noise.hip", "qn_ess.hip", "qn_nuts.hip", "qn_nuts_adapt.hip", "qn_rnet.hip", "qn_curv.hip", "qn_glm.hip", "qn_sobolev.hip", "qn_swag.hip", "qn_kron.hip", "qn_diag.hip", "qn_score.hip", "qn_psis.hip", "qn_stack.hip", "qn_rank.hip", "qn_evidence.hip", "qn_quantile.hip"]
# sources that #include another source (the second object of a file compiled in two parts): rebuilt when that one changes
SOURCE_DEPS = {"qn_wide_u_i8.hip": ["qn_wide_i8.hip"], "qn_fused_d8.hip": ["qn_fused.hip"], "qn_fused_o16.hip": ["qn_fused.hip"]}

HEADER = os.path.join(_HERE, "..", "include", "quinn_amd.h")       # the one place a signature or a code is written
PSIS_HEADER = os.path.join(_HERE, "..", "include", "quinn_amd_psis.h")    # ... and the PSIS-LOO extension's (csrc/qn_psis.hip)
STACK_HEADER = os.path.join(_HERE, "..", "include", "quinn_amd_stack.h")  # ... and the stacking extension's (csrc/qn_stack.hip)
RANK_HEADER = os.path.join(_HERE, "..", "include", "quinn_amd_rank.h")    # ... and the rank-diagnostics extension's (csrc/qn_rank.hip)
EV_HEADER = os.path.join(_HERE, "..", "include", "quinn_amd_evidence.h")  # ... and the Laplace-evidence extension's (csrc/qn_evidence.hip)
QUANT_HEADER = os.path.join(_HERE, "..", "include", "quinn_amd_quantile.h")  # ... and the predictive-quantile extension's (csrc/qn_quantile.hip)
NUTS_ADAPT_HEADER = os.path.join(_HERE, "..", "include", "quinn_amd_nuts_adapt.h")  # ... and the NUTS warm-up extension's (csrc/qn_nuts_adapt.hip)


class QuinnAmdError(RuntimeError):
    pass


_SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64,
            "double": ctypes.c_double, "size_t": ctypes.c_size_t}
_INT = r"(-?(?:0[xX][0-9a-fA-F]+|\d+))"


def _ctype(decl, ret, where):
    """The ctypes type of the C type `decl` (`where`: function and text, for the message).  Every pointer parameter is a
    c_void_p -- it takes None, an address, a ctypes array or byref() -- and a returned `const char*` a c_char_p."""
    words = [w for w in decl.replace("*", " * ").split() if w != "const"]
    if ret and words == ["void"]:
        return None
    if ret and words == ["char", "*"]:
        return ctypes.c_char_p
    if not ret and "*" in words:
        return ctypes.c_void_p
    if len(words) != 1 or words[0] not in _SCALARS:
        raise QuinnAmdError(f"{where}: unknown type '{decl.strip()}'")
    return _SCALARS[words[0]]


def parse_header(text):
    """(functions, constants) of the text of a C header.  functions: name -> (restype, [argtypes]) of every qn_* prototype, in
    the order of declaration; constants: name -> value of every `#define QN_X <integer>` and `enum { QN_X = <integer>, ... }`
    member.  Strict: a type that is neither in _SCALARS nor a pointer, a parameter without a name, or a `qn_name(` in a
    declaration of any other shape raises QuinnAmdError."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    constants = {k: int(v, 0) for k, v in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(QN_\w+)[ \t]+" + _INT + r"[ \t]*$", text, re.M)}
    for body in re.findall(r"\benum\s*\{([^}]*)\}", text):
        constants.update((k, int(v, 0)) for k, v in re.findall(r"\b(QN_\w+)\s*=\s*" + _INT + r"\s*(?:,|$)", body))
    text = re.sub(r"^[ \t]*#[^\n]*", " ", text, flags=re.M)
    functions = {}

    def prototype(m):
        ret, name, params = m.group(1), m.group(2), " ".join(m.group(3).split())
        argtypes = []
        for par in ([] if params == "void" else [par.strip() for par in params.split(",")]):
            split = re.fullmatch(r"(\S.*?)\s*\b(\w+)", par)
            if not split:
                raise QuinnAmdError(f"{name}({params}): no type and name in '{par}'")
            argtypes.append(_ctype(split.group(1), False, f"{name}({params}), parameter '{par}'"))
        functions[name] = (_ctype(ret, True, f"{name}, return"), argtypes)
        return " "

    rest = re.sub(r"([A-Za-z_][\w\s*]*?)\b(qn_\w+)\s*\(([^()]*)\)\s*;", prototype, text)
    left = re.search(r"\b(qn_\w+)\s*\(", rest)
    if left:
        raise QuinnAmdError(f"{left.group(1)}: not a plain prototype: '{' '.join(rest[left.start():].split(';')[0].split())}'")
    return functions, constants


with open(HEADER) as _f:
    FUNCTIONS, CONSTANTS = parse_header(_f.read())
SYMBOLS = list(FUNCTIONS)         # every symbol include/quinn_amd.h declares (tests check the .so exports all of them)
with open(PSIS_HEADER) as _f:
    PSIS_FUNCTIONS, _psis_constants = parse_header(_f.read())         # qn_psis_loo, its workspace query; QN_LOO_NOUT, QN_PSIS_MAX_M
with open(STACK_HEADER) as _f:
    STACK_FUNCTIONS, _stack_constants = parse_header(_f.read())       # qn_group_lpd, qn_stack_weights, qn_pred_score_w and their queries
with open(RANK_HEADER) as _f:
    RANK_FUNCTIONS, _rank_constants = parse_header(_f.read())         # qn_rank_diag, its workspace query; QN_RANK_MAX_S, QN_RANK_* rows
with open(EV_HEADER) as _f:
    EV_FUNCTIONS, _ev_constants = parse_header(_f.read())             # qn_la_evidence, qn_la_tune and their queries; QN_EV_*
with open(QUANT_HEADER) as _f:
    QUANT_FUNCTIONS, _quant_constants = parse_header(_f.read())       # qn_pred_quantile, its workspace query; QN_QUANT_MAX_M / _Q / _ITER
with open(NUTS_ADAPT_HEADER) as _f:
    NUTS_ADAPT_FUNCTIONS, _nuts_adapt_constants = parse_header(_f.read())   # qn_nuts_adapt; QN_NUTS_PLAN_*
QN_F64, QN_F32 = CONSTANTS["QN_F64"], CONSTANTS["QN_F32"]
# keyed by the reference's activation names (quinn/nns/mlp.py:46-84)
ACT_CODES = {"identity": CONSTANTS["QN_ACT_IDENTITY"], "tanh": CONSTANTS["QN_ACT_TANH"], "relu": CONSTANTS["QN_ACT_RELU"]}
# PATH_AUTO .., ARITH_PLAIN .., CURV_HESS_FULL .., GLM_COV_FULL .., SWAG_INIT .., SCORE_LPPD .. SCORE_NOUT, LOO_NOUT, PSIS_MAX_M, RANK_MAX_S, QUANT_MAX_M .., NUTS_PLAN_COLLECT ..: the headers'
# codes of these families under their names without the QN_ prefix
globals().update((k[3:], v) for k, v in list(CONSTANTS.items()) + list(_psis_constants.items()) + list(_stack_constants.items()) +
                 list(_rank_constants.items()) + list(_ev_constants.items()) + list(_quant_constants.items()) +
                 list(_nuts_adapt_constants.items())
                 if k.startswith(("QN_PATH_", "QN_ARITH_", "QN_CURV_", "QN_GLM_", "QN_SWAG_", "QN_SCORE_", "QN_LOO_", "QN_PSIS_",
                                  "QN_STACK_", "QN_RANK_", "QN_EV_", "QN_QUANT_", "QN_NUTS_")))


def build(force=False, verbose=False, jobs=None):
    """Compile the HIP sources for gfx950 into quinn_amd/lib/libquinn_amd.so (hipcc
    cross-compiles without a GPU).  One object per source under quinn_amd/lib/obj/, compiled in
    parallel and only when the source or a header is newer than its object; then one link.
    With QN_HIPCC_FLAGS set (A/B builds, -DQN_...) objects and library go to their OWN directory / file name, keyed by the
    flags (quinn_amd/lib/obj_<key>/, libquinn_amd_<key>.so; select the result with QUINN_AMD_LIB): a flagged build never
    replaces or poisons the default library.  Concurrent callers (ranks, pytest-xdist) are serialised by a file lock."""
    import fcntl
    import hashlib
    from concurrent.futures import ThreadPoolExecutor
    srcs = [os.path.join(CSRC, s) for s in SOURCES]
    hdrs = [os.path.join(CSRC, h) for h in sorted(os.listdir(CSRC)) if h.endswith(".h")] + \
           [HEADER, PSIS_HEADER, STACK_HEADER, RANK_HEADER, EV_HEADER, QUANT_HEADER, NUTS_ADAPT_HEADER]
    hnew = max(os.path.getmtime(h) for h in hdrs)
    extra = os.environ.get("QN_HIPCC_FLAGS", "").split()          # A/B builds (-DQN_...)
    key = hashlib.sha1(" ".join(extra).encode()).hexdigest()[:10] if extra else ""
    libpath = os.path.join(LIBDIR, f"libquinn_amd_{key}.so") if extra else LIBPATH
    objdir = os.path.join(LIBDIR, f"obj_{key}" if extra else "obj")
    os.makedirs(objdir, exist_ok=True)
    with open(os.path.join(LIBDIR, ".build.lock"), "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        if not force and os.path.exists(libpath):
            if os.path.getmtime(libpath) >= max(hnew, max(os.path.getmtime(s) for s in srcs)):
                return libpath
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        # -amdgpu-mfma-vgpr-form: keep MFMA accumulators in VGPRs (gfx950 has one unified register file);
        # without it hipcc copies every loop-carried accumulator VGPR<->AGPR per iteration (25 % of the GEMM loop)
        flags = ["-O3", "--offload-arch=gfx950", "-std=c++17", "-mllvm", "-amdgpu-mfma-vgpr-form", "-fPIC"]

        def one(src):
            obj = os.path.join(objdir, os.path.basename(src)[:-4] + ".o")
            newest = max([hnew, os.path.getmtime(src)] +
                         [os.path.getmtime(os.path.join(CSRC, dep)) for dep in SOURCE_DEPS.get(os.path.basename(src), [])])
            if not force and os.path.exists(obj) and os.path.getmtime(obj) >= newest:
                return obj
            cmd = [hipcc] + flags + extra + ["-c", src, "-o", obj]
            if verbose:
                print(" ".join(cmd), flush=True)
            subprocess.run(cmd, check=True)
            return obj

        with ThreadPoolExecutor(max_workers=jobs or min(8, os.cpu_count() or 1)) as ex:
            objs = list(ex.map(one, srcs))
        cmd = [hipcc, "--offload-arch=gfx950", "-fPIC", "-shared", "-o", libpath] + objs
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.run(cmd, check=True)
    return libpath


_lib = None


def lib():
    """The loaded library (loads on first use; raises QuinnAmdError if it is not built)."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("QUINN_AMD_LIB", LIBPATH)      # A/B builds of the kernels (tools/ab_build.sh)
    if not os.path.exists(path):
        raise QuinnAmdError(f"{path} not found: run `python -c 'import __graft_entry__ as g; g.build()'` "
                            "(hipcc --offload-arch=gfx950); there is no CPU fallback")
    L = ctypes.CDLL(path)
    for name, (restype, argtypes) in list(FUNCTIONS.items()) + list(PSIS_FUNCTIONS.items()) + list(STACK_FUNCTIONS.items()) + \
            list(RANK_FUNCTIONS.items()) + list(EV_FUNCTIONS.items()) + list(QUANT_FUNCTIONS.items()) + \
            list(NUTS_ADAPT_FUNCTIONS.items()):
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = L
    return L


def stream(dev=None):
    """The current torch stream of the device, as the C ABI takes it."""
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def check(rc, what):
    if rc != 0:
        raise QuinnAmdError(f"{what} failed (code {rc}): {lib().qn_last_error().decode()}")
