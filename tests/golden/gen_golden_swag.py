#!/usr/bin/env python3
"""Generate the SWAG fixtures tests/golden/g15_swag_*.npz by IMPORTING the reference (companion of gen_golden.py).

Runs only where the reference is importable; the tests read the committed .npz files:

    cd /tmp && QUINN_REFERENCE=<reference checkout> MPLBACKEND=Agg PYTHONDONTWRITEBYTECODE=1 \
        python3 <repo>/tests/golden/gen_golden_swag.py

  g15_swag_mlp_lowrank.npz   MLP (1,8,8,1) tanh, 3 members, k=3, n_steps=8, c=2 (4 collections: the deviation ring wraps)
  g15_swag_mlp_diag.npz      MLP (2,6,5,1) tanh, 4 members, diagonal covariance, n_steps=5, c=1
  g15_swag_rnet_lowrank.npz  the RNet of examples/ex_ufit.py at its SWAG settings (3 members, k=10, n_steps=12, c=1)

Each records seeds, w0, data, the member rows, the weight trajectory of the SWAG phase (`traj` [nens, n_steps + 1, p]: the
final MAP weights, then the weights after every SGD step), means, cov_diags, d_mats, and two predict_ens calls after a
recorded np.random.seed (no reseed in between): member indices, the thetas, the predictions and the means after each call.
Every saved cov_diags entry is asserted >= 0 (near-zero variances may change sign between two correct implementations).
"""
import os
import sys
import tempfile

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("QUINN_REFERENCE", "")
if REF and REF not in sys.path:
    sys.path.insert(0, REF)
os.environ.setdefault("MPLBACKEND", "Agg")
os.chdir(tempfile.mkdtemp(prefix="quinn_golden_"))      # nnfit drops PNGs into the CWD

from quinn.nns.mlp import MLP                            # noqa: E402
from quinn.nns import rnet as R                          # noqa: E402
from quinn.nns.nnwrap import NNWrap                      # noqa: E402
from quinn.ens.learner import Learner                    # noqa: E402
from quinn.solvers.nn_swag import NN_SWAG                # noqa: E402

VERS = np.array([torch.__version__, np.__version__])
torch.set_default_dtype(torch.double)


def data(N, d, o, noise, seed):
    rs = np.random.RandomState(seed)
    x = (rs.rand(N, d) * 2 - 1) * np.pi
    y = np.stack([np.sum(np.sin((k + 1) * x), axis=1) for k in range(o)], axis=1) + noise * rs.randn(N, o)
    return x, y


def save(name, **kw):
    np.savez_compressed(os.path.join(OUT, name), versions=VERS, **kw)
    print("wrote", name, {k: np.asarray(v).shape for k, v in kw.items()})


def flat(net):
    return NNWrap(net).p_flatten().detach().numpy().flatten()


def run(name, net, x, y, xv, yv, swag_kw, fit_kw, nens, dfrac, seeds, xpred, npred, **extra):
    w0 = flat(net)
    sw = NN_SWAG(net, nens=nens, dfrac=dfrac, verbose=False, **swag_kw)
    # weight trajectory of the SWAG phase: the weights after every one-epoch SGD fit of swag_calc
    traj = [[] for _ in range(nens)]
    member = {}
    orig_fit, orig_calc = Learner.fit, NN_SWAG.swag_calc

    def fit_rec(self, *a, **k):
        orig_fit(self, *a, **k)
        if k.get("optimizer") == "sgd" and k.get("nepochs") == 1:
            traj[member[id(self)]].append(flat(self.nnmodel))

    def calc_rec(self, learner, *a, **k):
        member[id(learner)] = j = len(self.means)
        traj[j].append(flat(learner.nnmodel))
        return orig_calc(self, learner, *a, **k)
    Learner.fit, NN_SWAG.swag_calc = fit_rec, calc_rec
    np.random.seed(seeds[0])
    torch.manual_seed(seeds[1])
    try:
        sw.fit(x, y, val=[xv, yv], freq_out=1000, **fit_kw)
    finally:
        Learner.fit, NN_SWAG.swag_calc = orig_fit, orig_calc
    np.random.seed(seeds[0])
    ntrn = x.shape[0]
    rows = np.stack([np.random.permutation(ntrn)[:int(ntrn * dfrac)] for _ in range(nens)])
    means = np.array(sw.means)
    cov_diags = np.array(sw.cov_diags)
    assert np.all(cov_diags >= 0), (name, cov_diags.min())
    d_mats = np.array(sw.d_mats) if sw.cov_type == "lowrank" else np.zeros((0,))
    # predictions: record randint and the weights handed to NNWrap.predict, in order
    jens, thetas = [], []
    o_ri, o_pred = np.random.randint, NNWrap.predict

    def ri(*a, **k):
        v = o_ri(*a, **k)
        jens.append(v)
        return v

    def pred(self, x_in, weights):
        thetas.append(np.array(weights, dtype=np.float64))
        return o_pred(self, x_in, weights)
    np.random.randint, NNWrap.predict = ri, pred
    np.random.seed(seeds[2])
    preds, means_after, js, ths = [], [], [], []
    try:
        for _ in range(2):
            jens.clear()
            thetas.clear()
            preds.append(np.array(sw.predict_ens(xpred, nens=npred)))
            means_after.append(np.array(sw.means))
            js.append(np.array(jens))
            ths.append(np.array(thetas))
    finally:
        np.random.randint, NNWrap.predict = o_ri, o_pred
    save(name, x=x, y=y, xval=xv, yval=yv, w0=w0, nens=nens, dfrac=dfrac, np_seed=seeds[0], torch_seed=seeds[1],
         pred_seed=seeds[2], rows=rows, traj=np.array(traj), means=means, cov_diags=cov_diags, d_mats=d_mats,
         k=swag_kw["k"], n_steps=swag_kw["n_steps"], c=swag_kw["c"], cov_type=np.array(swag_kw["cov_type"]),
         lr_swag=swag_kw["lr_swag"], datanoise=swag_kw["datanoise"], xpred=xpred, npred=npred,
         pred_jens=np.array(js), pred_thetas=np.array(ths), pred=np.array(preds), means_after=np.array(means_after),
         **{k: v for k, v in fit_kw.items() if v is not None}, **extra)


def mlp_cases():
    torch.manual_seed(160)
    net = MLP(1, 1, (8, 8), activ="tanh")
    x, y = data(30, 1, 1, 0.05, 161)
    xv, yv = data(8, 1, 1, 0.05, 162)
    run("g15_swag_mlp_lowrank.npz", net, x, y, xv, yv,
        dict(k=3, n_steps=8, c=2, cov_type="lowrank", lr_swag=0.05, datanoise=0.1, priorsigma=0.5),
        dict(lrate=0.01, batch_size=8, nepochs=15), nens=3, dfrac=0.8, seeds=(163, 164, 165),
        xpred=np.linspace(-3, 3, 9)[:, None], npred=5, dims=np.array((1, 8, 8, 1)), activ=np.array("tanh"))
    torch.manual_seed(170)
    net = MLP(2, 1, (6, 5), activ="tanh")
    x, y = data(26, 2, 1, 0.05, 171)
    xv, yv = data(6, 2, 1, 0.05, 172)
    run("g15_swag_mlp_diag.npz", net, x, y, xv, yv,
        dict(k=2, n_steps=5, c=1, cov_type="diag", lr_swag=0.05, datanoise=0.2, priorsigma=1.0),
        dict(lrate=0.02, batch_size=None, nepochs=10), nens=4, dfrac=0.9, seeds=(173, 174, 175),
        xpred=np.random.RandomState(176).rand(7, 2) * 4 - 2, npred=6, dims=np.array((2, 6, 5, 1)),
        activ=np.array("tanh"))


def rnet_case():
    # examples/ex_ufit.py: data, network and the SWAG settings of its 'swag' branch (8 MAP epochs: Adam
    # amplifies last-bit gradient differences of near-zero components over many updates)
    np.random.seed(180)
    torch.manual_seed(181)
    ndim, nall, datanoise = 1, 15, 0.02
    xall = np.random.rand(nall, ndim) * 2 * np.pi - np.pi
    yall = np.sum(np.sin(xall), axis=1).reshape(-1, 1) + datanoise * np.random.randn(nall, 1)
    ntrn = int(0.9 * nall)
    net = R.RNet(3, 3, wp_function=R.Poly(0), indim=ndim, outdim=1, layer_pre=True, layer_post=True, biasorno=True,
                 nonlin=True, mlp=False, final_layer=None)
    run("g15_swag_rnet_lowrank.npz", net, xall[:ntrn], yall[:ntrn], xall[ntrn:], yall[ntrn:],
        dict(k=10, n_steps=12, c=1, cov_type="lowrank", lr_swag=0.01, datanoise=0.1, priorsigma=1.0),
        dict(lrate=0.01, batch_size=2, nepochs=8), nens=3, dfrac=1.0, seeds=(182, 183, 184),
        xpred=np.linspace(-np.pi, np.pi, 11)[:, None], npred=7, rdim=3, nlayers=3, wp_kind=np.array("poly"), wp_arg=0,
        indim=ndim, outdim=1, biasorno=True, nonlin=True, mlp=False, layer_pre=True, layer_post=True)


if __name__ == "__main__":
    mlp_cases()
    rnet_case()
