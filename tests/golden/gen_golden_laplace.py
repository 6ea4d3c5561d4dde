#!/usr/bin/env python3
"""Generate the Laplace fixtures tests/golden/g14_*.npz by IMPORTING the reference (companion of gen_golden.py).

Runs only where the reference is importable; the GPU tests read the committed .npz files:

    cd /tmp && QUINN_REFERENCE=<reference checkout> MPLBACKEND=Agg PYTHONDONTWRITEBYTECODE=1 \
        python3 <repo>/tests/golden/gen_golden_laplace.py

  g14_hess_<k>.npz      NNWrap.calc_hess_full / calc_hess_diag (NegLogPost(net, N, sigma, None)) for 5 architectures
  g14_laplace_<t>.npz   NN_Laplace end to end for la_type t = full / diag: seeds, w0, data, means, the Hessians la_calc
                        formed, cov_mats, and predict_ens after a recorded np.random.seed (member indices and weight draws);
                        also la_calc(batch_size=7) of member 0 at its MAP weights on its rows
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
from quinn.nns.nnwrap import NNWrap                      # noqa: E402
from quinn.nns.losses import NegLogPost                  # noqa: E402
from quinn.solvers.nn_laplace import NN_Laplace          # noqa: E402

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


# ---------------------------------------------------------------- (a) Hessians of NNWrap
def hess_cases():
    cases = [(1, 1, (8, 8), "tanh", True, 40), (2, 1, (6, 5), "relu", True, 30), (3, 2, (5, 4), "identity", True, 25),
             (2, 2, (7, 6), "tanh", False, 33), (3, 2, (9,), "tanh", True, 20)]
    for k, (d, o, hls, act, bias, N) in enumerate(cases):
        torch.manual_seed(140 + k)
        net = MLP(d, o, hls, biasorno=bias, activ=act)
        w = flat(net)
        x, y = data(N, d, o, 0.1, 141 + k)
        sigma = 0.1 * (k + 1)
        nw = NNWrap(net)
        loss = NegLogPost(net, N, sigma, None)
        hf = nw.calc_hess_full(w, loss, x, y)
        hd = nw.calc_hess_diag(w, loss, x, y)
        save(f"g14_hess_{k}.npz", dims=np.array((d,) + hls + (o,)), activ=np.array(act), bias=bias, w=w, x=x, y=y,
             sigma=sigma, hess_full=hf, hess_diag=np.diag(hd), diag_offdiag_zero=bool(np.count_nonzero(hd - np.diag(np.diag(hd))) == 0))


# ---------------------------------------------------------------- (b), (c) NN_Laplace end to end
def laplace_run(la_type):
    d, o, hls, act, N = 1, 1, (8, 8), "tanh", 30
    torch.manual_seed(150)
    net = MLP(d, o, hls, activ=act)
    w0 = flat(net)
    x, y = data(N, d, o, 0.05, 151)
    xv, yv = data(8, d, o, 0.05, 152)
    hess = []
    orig = {"full": NNWrap.calc_hess_full, "diag": NNWrap.calc_hess_diag}[la_type]

    def rec(self, *a, **k):
        h = orig(self, *a, **k)
        hess.append(np.array(h))
        return h
    setattr(NNWrap, "calc_hess_" + la_type, rec)
    la = NN_Laplace(net, la_type=la_type, cov_scale=0.7, nens=3, dfrac=0.8, verbose=False, datanoise=0.1, priorsigma=0.5)
    np.random.seed(153)
    torch.manual_seed(154)
    la.fit(x, y, val=[xv, yv], lrate=0.01, batch_size=8, nepochs=15, freq_out=1000)
    hess_fit = np.array(hess)
    # the rows member j trained on: replay the permutations of the same seed
    np.random.seed(153)
    rows = np.stack([np.random.permutation(N)[:int(N * 0.8)] for _ in range(3)])
    # prediction draws: record randint and multivariate_normal results in order
    jens, thetas = [], []
    o_ri, o_mvn = np.random.randint, np.random.multivariate_normal

    def ri(*a, **k):
        v = o_ri(*a, **k)
        jens.append(v)
        return v

    def mvn(*a, **k):
        v = o_mvn(*a, **k)
        thetas.append(v)
        return v
    np.random.randint, np.random.multivariate_normal = ri, mvn
    xg = np.linspace(-3, 3, 9)[:, None]
    np.random.seed(155)
    try:
        ypred = la.predict_ens(xg, nens=6)
    finally:
        np.random.randint, np.random.multivariate_normal = o_ri, o_mvn
    # (c) la_calc with batches of 7 rows, member 0 on its own rows
    hess.clear()
    m0 = la.learners[0]
    NNWrap(m0.nnmodel).p_unflatten(la.means[0])      # predict_sample left a drawn theta in the member's module
    try:
        la.la_calc(m0, x[rows[0]], y[rows[0]], batch_size=7)
        batch_cov = la.cov_mats[3]
    except np.linalg.LinAlgError:                       # the reference's inverse of the summed batches can be singular
        batch_cov = np.zeros(0)
    hess_batches = np.array(hess)
    batched = hess_batches.sum(axis=0) if la_type == "full" else None
    setattr(NNWrap, "calc_hess_" + la_type, orig)
    save(f"g14_laplace_{la_type}.npz", dims=np.array((d,) + hls + (o,)), activ=np.array(act), x=x, y=y, xval=xv, yval=yv,
         w0=w0, nens=3, dfrac=0.8, lrate=0.01, batch_size=8, nepochs=15, np_seed=153, torch_seed=154, datanoise=0.1,
         priorsigma=0.5, cov_scale=0.7, rows=rows, means=np.array(la.means[:3]), hessians=hess_fit,
         cov_mats=np.array(la.cov_mats[:3]), pred_seed=155, xpred=xg, pred_jens=np.array(jens), pred_thetas=np.array(thetas),
         pred=np.array(ypred), batch_k=7, batch_hessians=hess_batches, batch_cov=batch_cov,
         **({} if batched is None else {"batch_sum": batched}))


if __name__ == "__main__":
    hess_cases()
    laplace_run("full")
    laplace_run("diag")
