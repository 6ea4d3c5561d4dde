"""GPU: every kernel family of the core operator (qn_mlp_sse_fwd / qn_mlp_sse_fwdbwd through the C ABI) stays inside the
workspace its size query asks for, computes the same bits in a larger one and refuses a smaller one.

One network per family (the NETS of tests/golden/gen_golden_sse_ws_sizes.py, whose CPU test checks that each reaches its family)
at B = 3 members -- odd: the XCD-aware grid is padded -- and 70 rows: above 64 and no multiple of 16 or 64, so the stashes' row
stride differs from the row count, the int8 weight gradient has a float64 tail and the last row split is ragged."""
import os
import sys

import pytest
import torch

from quinn_amd import _lib

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from gen_golden_sse_ws_sizes import NETS, make_desc   # noqa: E402

pytestmark = pytest.mark.gpu

B, ROWS, TAIL, FILL = 3, 70, 4096, 0xA5
EWORKSPACE = -2


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


def _data(L, h, net):
    """(W [B, p], X [rows, d], Y [rows, o]) float64 on the device, the same for every call of a case."""
    d, hid, o = (net["mlp"][0][0], max(net["mlp"][0][1:]), net["mlp"][0][-1]) if "mlp" in net else \
                (net["rnet"]["indim"], net["rnet"]["rdim"], net["rnet"]["outdim"])
    gen = torch.Generator().manual_seed(18)
    W = torch.randn(B, L.qn_mlp_num_params(h), generator=gen, dtype=torch.float64) / hid ** 0.5
    X = torch.rand(ROWS, d, generator=gen, dtype=torch.float64) * 2 - 1
    Y = torch.rand(ROWS, o, generator=gen, dtype=torch.float64)
    return W.cuda(), X.cuda(), Y.cuda(), o


def _call(L, h, grad, W, X, Y, o, ws, ws_bytes):
    """One call with `ws_bytes` of the buffer `ws` declared: (return code, sse, pred, grad or None)."""
    sse = torch.zeros(B, dtype=torch.float64, device="cuda")
    pred = torch.zeros(B, ROWS, o, dtype=torch.float64, device="cuda")
    st = _lib.stream()
    head = (h, _lib.QN_F64, W.data_ptr(), X.data_ptr(), Y.data_ptr(), None, B, ROWS, ROWS, sse.data_ptr(), pred.data_ptr())
    if grad:
        g = torch.zeros_like(W)
        rc = L.qn_mlp_sse_fwdbwd(*head, g.data_ptr(), ws.data_ptr(), ws_bytes, st)
    else:
        g = None
        rc = L.qn_mlp_sse_fwd(*head, ws.data_ptr(), ws_bytes, st)
    torch.cuda.synchronize()
    return rc, sse, pred, g


@pytest.mark.parametrize("grad", [0, 1], ids=["forward", "gradient"])
@pytest.mark.parametrize("name", list(NETS))
def test_family_stays_inside_its_workspace(L, name, grad):
    h = make_desc(L, NETS[name])
    W, X, Y, o = _data(L, h, NETS[name])
    need = L.qn_workspace_bytes(h, B, ROWS, grad, _lib.QN_F64)
    assert need > 0
    ws = torch.full((need + TAIL,), FILL, dtype=torch.uint8, device="cuda")
    rc, sse, pred, g = _call(L, h, grad, W, X, Y, o, ws, need)
    assert rc == 0, L.qn_last_error()
    assert bool((ws[need:] == FILL).all()), "wrote behind the workspace the size query asked for"
    assert bool(torch.isfinite(sse).all()) and bool((sse > 0).all())
    # the same call in a workspace twice as large: the kernels sum in a fixed order, so the results are the same bits
    big = torch.full((2 * need,), FILL, dtype=torch.uint8, device="cuda")
    rc2, sse2, pred2, g2 = _call(L, h, grad, W, X, Y, o, big, 2 * need)
    assert rc2 == 0, L.qn_last_error()
    assert torch.equal(sse, sse2) and torch.equal(pred, pred2)
    if grad:
        assert torch.equal(g, g2) and bool(torch.isfinite(g).all())
    # a workspace declared too small is refused before anything is launched.  256 bytes are too few for every family but one:
    # the forward of the fused residual-network kernels needs exactly one 256-byte block here (B x 1 partial sums), so its
    # exact fit must run and one byte less must be refused
    exact_fit = name == "rnet_fused" and not grad
    rc3, sse3, pred3, _ = _call(L, h, grad, W, X, Y, o, ws, 256)
    if exact_fit:
        assert rc3 == 0 and torch.equal(sse, sse3) and torch.equal(pred, pred3)
        rc3 = _call(L, h, grad, W, X, Y, o, ws, 255)[0]
    assert rc3 == EWORKSPACE and b"workspace" in L.qn_last_error()
    assert bool((ws[need:] == FILL).all())
    L.qn_mlp_desc_destroy(h)
