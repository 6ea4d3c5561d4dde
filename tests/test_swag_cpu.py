"""CPU: the SWAG recurrences (csrc/qn_swag.hip) restated in numpy against the reference's recorded runs
(tests/golden/g15_swag_*.npz), the prediction draw replay of NN_SWAG with the reference's in-place mean drift, the torch
permutation order of the two fit phases, and the argument checks (no device needed)."""
import os

import numpy as np
import pytest
import torch

from conftest import load_golden
from quinn_amd import _lib
from quinn_amd.nns.mlp import MLP
from quinn_amd.nns.nnfit import draw_perms
from quinn_amd.ops import check_swag_args
from quinn_amd.solvers import NN_SWAG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["g15_swag_mlp_lowrank.npz", "g15_swag_mlp_diag.npz", "g15_swag_rnet_lowrank.npz"]


def swag_moments(traj, c, k, lowrank):
    """swag_calc (nn_swag.py:86-123) on a recorded weight trajectory [n_steps + 1, p], in the kernel's order of operations
    with a ring buffer of k deviation rows; returns (mean, diag, D (p, k) oldest column first or None)."""
    m1 = traj[0].copy()
    m2 = traj[0] * traj[0]
    ring = np.zeros((k, traj.shape[1]))
    n = 0
    for i in range(1, traj.shape[0]):
        if i % c == 0:
            n = i // c
            w = traj[i]
            m1 = (n * m1 + w) / (n + 1)
            m2 = (n * m2 + w * w) / (n + 1)
            ring[(n - 1) % k] = w - m1
    D = ring[[(n + t) % k for t in range(k)]].T if lowrank else None
    return m1, m2 - m1 * m1, D


def sample_np(means, diags, dmats, js, z1, z2, k, lowrank, drift=True):
    """predict_sample's theta (nn_swag.py:125-145) for a sequence of draws; with drift the means move in place."""
    thetas = []
    for s, j in enumerate(js):
        corr = np.sqrt(diags[j]) * z1[s]
        if lowrank:
            corr = np.sqrt(0.5) * corr + np.sqrt(0.5) * np.dot(dmats[j], z2[s]) / np.sqrt(k - 1)
        if drift:
            means[j] += corr
            thetas.append(means[j].copy())
        else:
            thetas.append(means[j] + corr)
    return np.array(thetas)


@pytest.mark.parametrize("name", CASES)
def test_recurrences_reproduce_reference_moments(name):
    g = load_golden(name)
    lowrank = str(g["cov_type"]) == "lowrank"
    k, c = int(g["k"]), int(g["c"])
    for j in range(int(g["nens"])):
        m, dg, D = swag_moments(g["traj"][j], c, k, lowrank)
        assert np.array_equal(m, g["means"][j]), (name, j)
        assert np.array_equal(dg, g["cov_diags"][j]), (name, j)
        if lowrank:
            assert np.array_equal(D, g["d_mats"][j]), (name, j)


def _solver(g):
    """An NN_SWAG with the fixture's sizes (the draws need only nens, nparams and k)."""
    sw = NN_SWAG(MLP(1, 1, (4,)), nens=int(g["nens"]), k=int(g["k"]), n_steps=int(g["n_steps"]), c=int(g["c"]),
                 cov_type=str(g["cov_type"]))
    sw.nparams = g["means"].shape[1]
    return sw


@pytest.mark.parametrize("name", CASES)
def test_draw_replay_and_drift_over_two_calls(name):
    g = load_golden(name)
    sw = _solver(g)
    lowrank = str(g["cov_type"]) == "lowrank"
    means = g["means"].copy()
    np.random.seed(int(g["pred_seed"]))
    for call in range(2):
        js, z1, z2 = sw._draws(int(g["npred"]))
        assert np.array_equal(js, g["pred_jens"][call]), (name, call)
        th = sample_np(means, g["cov_diags"], g["d_mats"], js, z1, z2, int(g["k"]), lowrank)
        np.testing.assert_allclose(th, g["pred_thetas"][call], rtol=1e-13, atol=1e-15)
        np.testing.assert_allclose(means, g["means_after"][call], rtol=1e-13, atol=1e-15)
    # the drift is real: a member drawn twice moved its mean between the draws
    assert not np.array_equal(g["means_after"][0], g["means"])


def test_draws_consume_z2_for_diagonal_covariance():
    g = load_golden("g15_swag_mlp_diag.npz")
    sw = _solver(g)
    np.random.seed(5)
    js, z1, z2 = sw._draws(3)
    np.random.seed(5)
    for s in range(3):
        assert np.random.randint(0, sw.nens) == js[s]
        assert np.array_equal(np.random.randn(sw.nparams), z1[s])
        assert np.array_equal(np.random.randn(sw.k), z2[s])


def test_draw_perms_split_is_reference_torch_order():
    nens, nepochs, n_steps, nsub = 3, 4, 5, 7
    torch.manual_seed(11)
    perms = draw_perms(nens, nepochs + n_steps, nsub)
    torch.manual_seed(11)
    for j in range(nens):                       # member j: its MAP epochs (nnfit), then swag_calc's one-epoch fits
        for t in range(nepochs):
            assert np.array_equal(perms[j, :nepochs][t], torch.randperm(nsub).numpy())
        for t in range(n_steps):
            assert np.array_equal(perms[j, nepochs:][t], torch.randperm(nsub).numpy())


@pytest.mark.parametrize("k,n_steps,c,cov_type", [(1, 12, 1, "lowrank"), (0, 12, 1, "diag"), (10, 12, 0, "lowrank"),
                                                  (10, -1, 1, "diag"), (10, 9, 1, "lowrank"), (10, 12, 2, "lowrank"),
                                                  (3, 8, 3, "lowrank"), (2.5, 12, 1, "lowrank"), (10, 12, 1.0, "diag")])
def test_bad_arguments_are_refused(k, n_steps, c, cov_type):
    with pytest.raises(ValueError):
        check_swag_args(k, n_steps, c, cov_type)
    with pytest.raises(ValueError):
        NN_SWAG(MLP(1, 1, (4,)), nens=2, k=k, n_steps=n_steps, c=c, cov_type=cov_type)


@pytest.mark.parametrize("k,n_steps,c,cov_type,lowrank", [(10, 12, 1, "lowrank", True), (3, 8, 2, "lowrank", True),
                                                          (10, 5, 3, "diag", False), (2, 0, 1, "anything", False)])
def test_good_arguments_are_accepted(k, n_steps, c, cov_type, lowrank):
    assert check_swag_args(k, n_steps, c, cov_type) is lowrank
    sw = NN_SWAG(MLP(1, 1, (4,)), nens=2, k=k, n_steps=n_steps, c=c, cov_type=cov_type)
    assert sw.means == [] and sw.cov_diags == [] and sw.d_mats == []


def test_entry_points_declared_and_listed():
    hdr = open(os.path.join(ROOT, "include", "quinn_amd.h")).read()
    for sym in ("qn_swag_step", "qn_swag_sample"):
        assert f"int {sym}(" in hdr
        assert sym in _lib.SYMBOLS
    assert "qn_swag.hip" in _lib.SOURCES
    assert (_lib.SWAG_INIT, _lib.SWAG_SGD, _lib.SWAG_SGD_COLLECT) == (0, 1, 2)
    for name, val in (("QN_SWAG_INIT", 0), ("QN_SWAG_SGD", 1), ("QN_SWAG_SGD_COLLECT", 2)):
        assert f"#define {name}" in hdr and hdr.split(f"#define {name}")[1].split()[0] == str(val)
