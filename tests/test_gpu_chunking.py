"""GPU: the member-chunked call of the float64 extension operators (BatchedMLP._run_chunked).  A member's result must not depend
on how the members are split over the C calls: an operator that takes all members in one call and one that takes a single member
per call (max_workspace_bytes=1) give the same bits.  Shapes: N = 7 is no multiple of 4, 16 or 64, B = 5 is odd (uneven halving),
two outputs, and the row subsets repeat and reorder rows -- the smallest at which a wrong slice, a stale workspace or a wrong
member pointer shows.  (The SSE operator's chunking goes by set_plan_batch: tests/fuzz_all.py.)"""
import numpy as np
import pytest
import torch

from quinn_amd.ops import MLPArch, BatchedMLP

pytestmark = pytest.mark.gpu

B, N, NB = 5, 7, 6


@pytest.fixture(scope="module")
def prob():
    arch = MLPArch((2, 5, 3, 2), "tanh", True)
    rs = np.random.RandomState(7)
    x, y, g = rs.randn(N, 2), rs.randn(N, 2), rs.randn(N, 2, 2)
    W = rs.randn(B, arch.nparams) / 2
    rows = rs.randint(0, N, size=(B, NB)).astype(np.int32)
    rows[:, :3] = [[6, 0, 6]] * B                                  # every member: a repeated row, out of order
    whole = BatchedMLP(arch, x, y, device="cuda:0")
    single = BatchedMLP(arch, x, y, device="cuda:0", max_workspace_bytes=1)
    for op in (whole, single):
        op.set_grad_data(g)
    # the premise: all members in one call / one member per call
    assert whole._fit_chunk(B, lambda bc: 4096 * bc, "query") == (B, 4096 * B)
    assert single._fit_chunk(B, lambda bc: 4096 * bc, "query") == (1, 4096)
    A, S, lay = whole.kron_factors(W, rows)
    UA, US, Dinv = torch.empty_like(A), torch.empty_like(S), torch.empty(B, arch.nparams, dtype=torch.float64, device=A.device)
    for i in range(len(arch.dims) - 1):
        la, ua = torch.linalg.eigh(lay.A(A, i))
        ls, us = torch.linalg.eigh(lay.S(S, i))
        lay.A(UA, i).copy_(ua)
        lay.S(US, i).copy_(us)
        lay.K(Dinv, i).copy_(1.0 / (ls[:, :, None] * la[:, None, :] / NB + 1.0))
    Sig = torch.as_tensor(rs.randn(B, arch.nparams, arch.nparams), device=A.device)
    Sig = Sig @ Sig.transpose(1, 2) / arch.nparams
    return dict(whole=whole, single=single, W=W, rows=rows, Sig=Sig, UA=UA, US=US, Dinv=Dinv)


CASES = {
    "glm_predict_full": lambda op, p: op.glm_predict(p["W"], p["Sig"]),
    "glm_predict_diag": lambda op, p: op.glm_predict(p["W"], torch.diagonal(p["Sig"], dim1=1, dim2=2).contiguous()),
    "kron_factors": lambda op, p: op.kron_factors(p["W"], p["rows"])[:2],
    "kron_glm_predict": lambda op, p: op.kron_glm_predict(p["W"], p["UA"], p["US"], p["Dinv"]),
    "input_jacobian": lambda op, p: op.input_jacobian(p["W"], want_pred=True),
    "sobolev": lambda op, p: op.sobolev(p["W"], 1.0, 0.37, row_idx=p["rows"], want_grad=True),
}


@pytest.mark.parametrize("case", list(CASES))
def test_result_does_not_depend_on_member_chunking(prob, case):
    a = CASES[case](prob["whole"], prob)
    b = CASES[case](prob["single"], prob)
    assert len(a) == len(b) >= 2
    for u, v in zip(a, b):
        assert u.shape[0] == B and torch.isfinite(u).all()
        assert torch.equal(u, v)
