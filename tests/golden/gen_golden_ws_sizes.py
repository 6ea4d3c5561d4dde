"""Records what the workspace-size queries of the float64 extension operators return (no device needed):

  g16_ext_workspace_bytes.json   qn_curv_workspace_bytes (four kinds), qn_glm_workspace_bytes (two kinds),
                                 qn_kron_workspace_bytes, qn_kron_glm_workspace_bytes, qn_sobolev_workspace_bytes (want_grad 0 / 1)
                                 for B in {1, 8}, rows in {1, 63, 5000} and three architectures (one without bias)

The committed file was written by the library as it stood BEFORE the host plumbing of these operators moved into
csrc/qn_host_args.h; tests/test_kron_cpu.py::test_extension_workspace_sizes_unchanged holds every later build to it.  Run it
again only when a workspace layout is changed on purpose:  python tests/golden/gen_golden_ws_sizes.py
"""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))

ARCHS = [((2, 5, 3, 2), "tanh", 1), ((1, 64, 64, 64, 1), "tanh", 1), ((3, 20, 7, 2), "relu", 0)]
MEMBERS = (1, 8)
ROWS = (1, 63, 5000)
# (query, leading arguments after the descriptor, trailing arguments after (B, rows))
QUERIES = [("qn_curv_workspace_bytes", (kind,), ()) for kind in (0, 1, 2, 3)] + \
          [("qn_glm_workspace_bytes", (kind,), ()) for kind in (0, 1)] + \
          [("qn_kron_workspace_bytes", (), ()), ("qn_kron_glm_workspace_bytes", (), ())] + \
          [("qn_sobolev_workspace_bytes", (), (want_grad,)) for want_grad in (0, 1)]


def cases(L):
    """[{query, dims, act, bias, args, bytes}] of every query x architecture x B x rows; args follow the descriptor."""
    from quinn_amd import _lib
    out = []
    for dims, act, bias in ARCHS:
        h = ctypes.c_void_p()
        rc = L.qn_mlp_desc_create((ctypes.c_int * len(dims))(*dims), len(dims), _lib.ACT_CODES[act], bias, ctypes.byref(h))
        assert rc == 0
        for query, lead, trail in QUERIES:
            for B in MEMBERS:
                for rows in ROWS:
                    args = list(lead) + [B, rows] + list(trail)
                    out.append({"query": query, "dims": list(dims), "act": act, "bias": bias, "args": args,
                                "bytes": int(getattr(L, query)(h, *args))})
        L.qn_mlp_desc_destroy(h)
    return out


if __name__ == "__main__":
    from quinn_amd import _lib
    _lib.build()
    rec = cases(_lib.lib())
    assert all(c["bytes"] > 0 for c in rec)
    with open(os.path.join(HERE, "g16_ext_workspace_bytes.json"), "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(c) for c in rec) + "\n]\n")          # one case per line
    print(len(rec), "cases")
