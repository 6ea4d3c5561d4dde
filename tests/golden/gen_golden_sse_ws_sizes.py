"""Records what the size queries of the core operator (qn_mlp_sse_fwd / _fwdbwd / _fwd_parts) return (no device needed):

  g18_sse_workspace_bytes.json   qn_workspace_bytes (want_grad 0 / 1) and qn_mlp_sse_parts for B in {1, 8, 300},
                                 rows in {1, 63, 64, 70, 5000}, float64 / float32, QN_PATH_AUTO / QN_PATH_GENERIC, once as is and
                                 once with qn_mlp_desc_set_plan_batch(d, 64), for one network per kernel family (NETS below)

The committed file was written by the library as it stood BEFORE every family's workspace layout moved into one function shared
by its size query and its run function; tests/test_host_api_errors.py::test_sse_workspace_sizes_unchanged holds every later
build to it.  Run it again only when a workspace layout is changed on purpose:  python tests/golden/gen_golden_sse_ws_sizes.py
"""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))

# name -> network and the kernel family it is here for: (qn_mlp_path, qn_mlp_arith) of the forward and of the gradient at
# B = 3, 70 rows, float64, QN_PATH_AUTO (1 = layer-wise, 2 = fused; arithmetic 0 plain, 1 fused int8, 2 wide int8, 3 int8 layers).
# "mlp": (dims, activation, bias); "rnet": the arguments of qn_rnet_desc_create after the coefficients are split off
NETS = {
    "fused_f64": {"mlp": [[1, 32, 32, 1], "relu", 1], "family": [[2, 0], [2, 0]]},
    "fused_i8": {"mlp": [[1, 64, 64, 1], "tanh", 1], "family": [[2, 1], [2, 1]]},
    "padded_fused": {"mlp": [[2, 33, 33, 1], "tanh", 1], "family": [[2, 1], [2, 1]]},
    "padded_generic": {"mlp": [[20, 50, 50, 2], "tanh", 1], "family": [[1, 0], [1, 0]]},
    "stream_128": {"mlp": [[2, 128, 1], "tanh", 1], "family": [[2, 0], [1, 0]]},
    "wide_i8_tanh_128": {"mlp": [[2, 128, 128, 1], "tanh", 1], "family": [[1, 2], [1, 2]]},
    "wide_i8_tanh_256": {"mlp": [[2, 256, 256, 1], "tanh", 1], "family": [[1, 2], [1, 2]]},
    "wide_i8_relu_128": {"mlp": [[2, 128, 128, 1], "relu", 1], "family": [[1, 2], [1, 2]]},
    "i8_layers": {"mlp": [[2, 128, 256, 1], "tanh", 1], "family": [[1, 3], [1, 3]]},
    "layerwise": {"mlp": [[20, 30, 7, 2], "relu", 0], "family": [[1, 0], [1, 0]]},
    "rnet_fused": {"rnet": {"indim": 1, "rdim": 3, "outdim": 1, "nsteps": 2, "npar": 1, "coef": [1.0, 1.0], "act": "tanh", "bias": 1,
                            "pre": 1, "post": 1, "mlp": 0}, "family": [[2, 0], [2, 0]]},
    "rnet_layerwise": {"rnet": {"indim": 2, "rdim": 12, "outdim": 2, "nsteps": 3, "npar": 2,
                                "coef": [1.0, 0.0, 1.0, 0.5, 1.0, 1.0], "act": "tanh", "bias": 1, "pre": 1, "post": 1, "mlp": 0},
                       "family": [[1, 0], [1, 0]]},
}
MEMBERS = (1, 8, 300)
ROWS = (1, 63, 64, 70, 5000)


def make_desc(L, net):
    """The descriptor of one NETS entry (the caller destroys it)."""
    from quinn_amd import _lib
    h = ctypes.c_void_p()
    if "mlp" in net:
        dims, act, bias = net["mlp"]
        rc = L.qn_mlp_desc_create((ctypes.c_int * len(dims))(*dims), len(dims), _lib.ACT_CODES[act], bias, ctypes.byref(h))
    else:
        r = net["rnet"]
        rc = L.qn_rnet_desc_create(r["indim"], r["rdim"], r["outdim"], r["nsteps"], r["npar"],
                                   (ctypes.c_double * len(r["coef"]))(*r["coef"]), _lib.ACT_CODES[r["act"]], r["bias"], r["pre"],
                                   r["post"], r["mlp"], ctypes.byref(h))
    assert rc == 0
    return h


def family(L, h):
    """[[path, arithmetic] of the forward, the same of the gradient] at B = 3, 70 rows, float64."""
    return [[int(L.qn_mlp_path(h, 3, 70, g, 0)), int(L.qn_mlp_arith(h, 3, 70, g, 0))] for g in (0, 1)]


def cases(L):
    """[{net, plan, path, dtype, B, rows, bytes: [forward, gradient], parts}] over the whole grid."""
    out = []
    for name, net in NETS.items():
        h = make_desc(L, net)
        for plan in (0, 64):
            L.qn_mlp_desc_set_plan_batch(h, plan)
            for path in (0, 1):
                L.qn_mlp_desc_set_path(h, path)
                for dtype in (0, 1):
                    for B in MEMBERS:
                        for rows in ROWS:
                            out.append({"net": name, "plan": plan, "path": path, "dtype": dtype, "B": B, "rows": rows,
                                        "bytes": [int(L.qn_workspace_bytes(h, B, rows, g, dtype)) for g in (0, 1)],
                                        "parts": int(L.qn_mlp_sse_parts(h, B, rows, dtype))})
        L.qn_mlp_desc_destroy(h)
    return out


if __name__ == "__main__":
    from quinn_amd import _lib
    _lib.build()
    L = _lib.lib()
    for name, net in NETS.items():
        h = make_desc(L, net)
        assert family(L, h) == net["family"], (name, family(L, h))
        L.qn_mlp_desc_destroy(h)
    rec = cases(L)
    assert all(min(c["bytes"]) > 0 and c["parts"] >= 1 for c in rec)
    with open(os.path.join(HERE, "g18_sse_workspace_bytes.json"), "w") as f:           # one net / one case per line
        f.write('{"nets": {\n' + ",\n".join(json.dumps(k) + ": " + json.dumps(v) for k, v in NETS.items()) + '\n},\n"cases": [\n' +
                ",\n".join(json.dumps(c) for c in rec) + "\n]}\n")
    print(len(rec), "cases")
