"""CPU: the Kronecker-factored Gauss-Newton (csrc/qn_kron.hip) restated in numpy -- factors, eigen-pair variances, dense
covariance, linearised predictive, sampler -- against torch.func Jacobians; the layout / workspace queries and refusals of the new
entry points (no device needed) and the argument checks of the 'kron' Laplace type."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from quinn_amd import _lib
from quinn_amd.ops import MLPArch, RNetArch, check_kron_args, kron_layout
from test_glm_cpu import CASES, jac_rows_np, jac_np, jac_autograd, _desc, _rnet


def kron_shapes(arch):
    """(e, h, offK, perm): e_i = h_i + bias, h_{i+1}, the kron-order offset of layer i, and perm with flat = perm[kron]."""
    hb = 1 if arch.bias else 0
    e = [d + hb for d in arch.dims[:-1]]
    h = list(arch.dims[1:])
    offK, perm, off = [], np.empty(arch.nparams, dtype=np.int64), 0
    for i, (ei, hi) in enumerate(zip(e, h)):
        offK.append(off)
        d = arch.dims[i]
        for a in range(hi):
            for c in range(ei):
                perm[off + a * ei + c] = off + a * d + c if c < d else off + hi * d + a
        off += hi * ei
    return e, h, offK, perm


def kron_factors_np(arch, w, x):
    """(A, S): per layer A_i = sum_n ~in_i ~in_i^T [e_i, e_i] and S_i = sum_n sum_k g^k_i g^k_i^T [h_{i+1}, h_{i+1}]."""
    _, ins, gk = jac_rows_np(arch, w, x)
    L = len(arch.dims) - 1
    A = [ins[i] @ ins[i].T for i in range(L)]
    S = [sum(gk[k][i] @ gk[k][i].T for k in range(arch.dims[-1])) for i in range(L)]
    return A, S


def kron_eig_np(M):
    """(eigenvalues clamped at 0, eigenvectors in the columns) per layer."""
    lam, U = zip(*[np.linalg.eigh(m) for m in M])
    return [np.maximum(v, 0.0) for v in lam], list(U)


def kron_dinv_np(lamS, lamA, nb, datanoise, priorsigma, cov_scale):
    """Per layer Dinv [h_{i+1}, e_i]: the variance of eigen-pair (a, c)."""
    return [1.0 / (cov_scale * (ls[:, None] * la[None, :] / (nb * datanoise ** 2) + 1.0 / priorsigma ** 2))
            for ls, la in zip(lamS, lamA)]


def kron_block_idx(arch, i):
    """Flat indices of layer i's parameters in kron order: a kron-order block sits at [idx][:, idx] of a flat-order matrix."""
    e, h, offK, perm = kron_shapes(arch)
    return perm[offK[i]:offK[i] + h[i] * e[i]]


def kron_dense_np(arch, blocks):
    """Block-diagonal [p, p] in flat order from per-layer kron-order blocks."""
    p = arch.nparams
    out = np.zeros((p, p))
    for i, blk in enumerate(blocks):
        idx = kron_block_idx(arch, i)
        out[np.ix_(idx, idx)] = blk
    return out


def kron_dense_cov_np(arch, US, UA, Dinv):
    blocks = []
    for us, ua, di in zip(US, UA, Dinv):
        Q = np.kron(us, ua)
        blocks.append((Q * di.reshape(-1)) @ Q.T)
    return kron_dense_np(arch, blocks)


def kron_dense_prec_np(arch, S, A, nb, datanoise, priorsigma, cov_scale):
    return kron_dense_np(arch, [cov_scale * (np.kron(s, a) / (nb * datanoise ** 2) + np.eye(len(s) * len(a)) / priorsigma ** 2)
                                for s, a in zip(S, A)])


def kron_glm_np(arch, w, x, US, UA, Dinv, absolute=False):
    """(f [N, o], cov [N, o, o]) by the kernel's formula; absolute=True evaluates it with |U_S|, |U_A|, |g|, |~in| (the
    magnitude the rounding-error bound is relative to)."""
    f, ins, gk = jac_rows_np(arch, w, x)
    ab = np.abs if absolute else (lambda v: v)
    N, o = x.shape[0], arch.dims[-1]
    cov = np.zeros((N, o, o))
    for i in range(len(US)):
        ah = ab(UA[i]).T @ ab(ins[i])                                          # [e, N]
        T = Dinv[i] @ (ah * ah)                                                # [h, N]
        gh = np.stack([ab(US[i]).T @ ab(gk[k][i]) for k in range(o)])          # [o, h, N]
        cov += np.einsum("kan,lan,an->nkl", gh, gh, T)
    return f, cov


def kron_sample_np(arch, mean, US, UA, Dih, z, absolute=False):
    """One draw in flat order: per layer mean + U_S (Z o Dih) U_A^T with Z[a][b] = z[flat position of (i, a, b)]."""
    e, h, offK, perm = kron_shapes(arch)
    ab = np.abs if absolute else (lambda v: v)
    out = np.zeros_like(mean) if absolute else mean.copy()
    for i in range(len(US)):
        idx = perm[offK[i]:offK[i] + h[i] * e[i]]
        Z = z[idx].reshape(h[i], e[i])
        out[idx] += (ab(US[i]) @ (ab(Z) * Dih[i]) @ ab(UA[i]).T).reshape(-1)
    return out


@pytest.mark.parametrize("dims,act,bias", CASES)
def test_kron_restatement_matches_autograd(dims, act, bias):
    arch = MLPArch(dims, act, bias)
    rs = np.random.RandomState(len(dims) * 100 + dims[-1])
    x = rs.randn(23, dims[0])
    w = rs.randn(arch.nparams) / np.sqrt(max(dims))
    p, L = arch.nparams, len(dims) - 1
    e, h, offK, perm = kron_shapes(arch)
    Jr = jac_autograd(arch, w, x)                                              # [N, o, p]
    # Nb = 1: every layer block of (S (x) A) / Nb is the block of J^T J
    A1, S1 = kron_factors_np(arch, w, x[:1])
    G1 = np.einsum("nkp,nkq->pq", Jr[:1], Jr[:1])
    for i in range(L):
        idx = perm[offK[i]:offK[i] + h[i] * e[i]]
        assert np.max(np.abs(np.kron(S1[i], A1[i]) - G1[np.ix_(idx, idx)])) <= 1e-12 * np.max(np.abs(G1))
    # Nb = 23: the last layer's block is exact
    A, S = kron_factors_np(arch, w, x)
    G = np.einsum("nkp,nkq->pq", Jr, Jr)
    idx = perm[offK[L - 1]:]
    assert np.max(np.abs(np.kron(S[L - 1], A[L - 1]) / 23 - G[np.ix_(idx, idx)])) <= 1e-12 * np.max(np.abs(G))
    assert np.max(np.abs(S[L - 1] - 23 * np.eye(dims[-1]))) <= 1e-12 * 23
    # eigen form of the covariance times the dense precision
    nb, dn, ps, cs = 23, 0.5, 1.3, 0.7
    lamS, US = kron_eig_np(S)
    lamA, UA = kron_eig_np(A)
    Dinv = kron_dinv_np(lamS, lamA, nb, dn, ps, cs)
    Sigma = kron_dense_cov_np(arch, US, UA, Dinv)
    H = kron_dense_prec_np(arch, S, A, nb, dn, ps, cs)
    assert np.max(np.abs(Sigma @ H - np.eye(p))) <= 1e-12
    # the predictive formula is J Sigma J^T
    f, C = kron_glm_np(arch, w, x, US, UA, Dinv)
    Cref = np.einsum("nkp,pq,nlq->nkl", Jr, Sigma, Jr)
    assert np.max(np.abs(C - Cref)) <= 1e-12 * np.max(np.abs(Cref))
    fj, J = jac_np(arch, w, x)
    assert np.array_equal(f, fj)
    # the sampler is mean + F z with F F^T = Sigma (through the factor matrix, no draws)
    Dih = [np.sqrt(d) for d in Dinv]
    mean = rs.randn(p)
    F = np.stack([kron_sample_np(arch, mean, US, UA, Dih, z) - mean for z in np.eye(p)], axis=1)
    assert np.max(np.abs(F @ F.T - Sigma)) <= 1e-12 * np.max(np.abs(Sigma))
    assert np.array_equal(kron_sample_np(arch, mean, US, UA, Dih, np.zeros(p)), mean)


@pytest.fixture(scope="module")
def L():
    _lib.build()
    return _lib.lib()


def _layout(L, h, n):
    arr = lambda: (ctypes.c_int64 * n)()                                       # noqa: E731
    oa, os_, ok = arr(), arr(), arr()
    la, ls = ctypes.c_int64(), ctypes.c_int64()
    rc = L.qn_kron_layout(h, oa, os_, ok, ctypes.byref(la), ctypes.byref(ls))
    return rc, list(oa), list(os_), list(ok), la.value, ls.value


@pytest.mark.parametrize("dims", [(1, 64, 64, 64, 1), (1, 128, 128, 1)])
def test_kron_layout_and_workspace_without_device(L, dims):
    h = _desc(L, dims)
    arch = MLPArch(dims)
    e, hh, offK, _ = kron_shapes(arch)
    rc, oa, os_, ok, la, ls = _layout(L, h, len(dims) - 1)
    assert rc == 0
    assert la == sum(v * v for v in e) and ls == sum(v * v for v in hh)
    assert oa == list(np.cumsum([0] + [v * v for v in e])[:-1]) and os_ == list(np.cumsum([0] + [v * v for v in hh])[:-1])
    assert ok == offK
    lay = kron_layout(arch, L)
    assert (lay.lenA, lay.lenS, list(lay.offK)) == (la, ls, offK) and np.array_equal(lay.perm, kron_shapes(arch)[3])
    assert L.qn_kron_workspace_bytes(h, 8, 4096) > 0
    N, o, p = 16384, 1, arch.nparams
    ws = L.qn_kron_glm_workspace_bytes(h, 1, N)
    assert 0 < ws < 8 * N * o * p                                              # bounded by a row tile, never N x p
    assert L.qn_kron_glm_workspace_bytes(h, 1, 4 * N) == ws
    assert L.qn_kron_workspace_bytes(h, 0, 10) == 0 and L.qn_kron_workspace_bytes(h, 1, 0) == 0
    if arch.nparams > 16384:                                                   # where the FULL kinds are refused
        assert L.qn_curv_workspace_bytes(h, _lib.CURV_GGN_FULL, 1, 100) == 0
        assert L.qn_glm_workspace_bytes(h, _lib.GLM_COV_FULL, 1, 100) == 0
    assert L.qn_mlp_kron_factors(h, None, None, None, 1, 10, 10, None, None, None, 0, None) == -1
    assert L.qn_mlp_kron_glm_predict(h, None, None, None, None, None, 1, 10, None, None, None, 0, None) == -1
    assert L.qn_kron_sample(h, None, None, None, None, None, None, None, 1, None) == -1
    L.qn_mlp_desc_destroy(h)


def test_kron_layout_without_bias(L):
    arch = MLPArch((2, 5, 9, 4), "tanh", False)
    h = _desc(L, arch.dims, bias=0)
    rc, oa, os_, ok, la, ls = _layout(L, h, 3)
    assert rc == 0 and la == 4 + 25 + 81 and ls == 25 + 81 + 16 and ok == [0, 10, 55]
    assert np.array_equal(kron_layout(arch, L).perm, np.arange(arch.nparams))  # kron order is the flat order without biases
    L.qn_mlp_desc_destroy(h)


def test_kron_refusals(L):
    rn = _rnet(L)
    assert L.qn_kron_workspace_bytes(rn, 1, 10) == 0
    assert b"RNet" in L.qn_last_error()
    assert L.qn_kron_glm_workspace_bytes(rn, 1, 10) == 0
    assert b"RNet" in L.qn_last_error()
    assert _layout(L, rn, 3)[0] == -1
    assert L.qn_mlp_kron_factors(rn, None, None, None, 1, 10, 10, None, None, None, 0, None) == -1
    assert L.qn_mlp_kron_glm_predict(rn, None, None, None, None, None, 1, 10, None, None, None, 0, None) == -1
    assert L.qn_kron_sample(rn, None, None, None, None, None, None, None, 1, None) == -1
    assert b"RNet" in L.qn_last_error()
    L.qn_mlp_desc_destroy(rn)
    wide = _desc(L, (1, 600, 1))
    assert L.qn_kron_workspace_bytes(wide, 1, 10) == 0
    assert b"width" in L.qn_last_error()
    L.qn_mlp_desc_destroy(wide)


def test_kron_argument_checks():
    from quinn_amd.solvers import NN_Laplace
    arch = MLPArch((1, 8, 1))
    assert check_kron_args(arch, "float64") is None
    with pytest.raises(ValueError, match="float64"):
        check_kron_args(arch, "float32")
    with pytest.raises(NotImplementedError, match="RNet"):
        check_kron_args(RNetArch(1, 3, 1, 2, ((1.0,), (1.0,))), "float64")
    net = torch.nn.Sequential(torch.nn.Linear(1, 4), torch.nn.Tanh(), torch.nn.Linear(4, 1)).double()
    assert NN_Laplace(net, la_type="kron", nens=1)._kind() == "kron"
    with pytest.raises(NotImplementedError):
        NN_Laplace(net, la_type="kfac", nens=1)._kind()


def test_extension_workspace_sizes_unchanged(L):
    """Every workspace-size query of the float64 extension operators (curvature, linearised predictive, Kronecker factors and
    predictive, input derivatives) returns what tests/golden/g16_ext_workspace_bytes.json records: the numbers of the library
    before the host plumbing of these operators was shared (gen_golden_ws_sizes.py), so the workspace layouts are unchanged."""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g16_ext_workspace_bytes.json")) as f:
        cases = json.load(f)
    queries = {c["query"] for c in cases}
    assert queries == {"qn_curv_workspace_bytes", "qn_glm_workspace_bytes", "qn_kron_workspace_bytes",
                       "qn_kron_glm_workspace_bytes", "qn_sobolev_workspace_bytes"} and len(cases) == 180
    descs = {}
    for c in cases:
        key = (tuple(c["dims"]), c["act"], c["bias"])
        if key not in descs:
            descs[key] = _desc(L, key[0], _lib.ACT_CODES[key[1]], key[2])
        assert c["bytes"] > 0
        assert getattr(L, c["query"])(descs[key], *c["args"]) == c["bytes"], c
    assert len(descs) == 3 and any(k[2] == 0 for k in descs)
    for h in descs.values():
        L.qn_mlp_desc_destroy(h)
