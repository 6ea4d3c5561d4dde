#!/usr/bin/env python
"""Fitting a surrogate to function values AND observed input gradients (adjoint / sensitivity data).

    python examples/ex_gradfit.py [--quick]

y = sin(x0) x1 on [-2, 2]^2 with its analytic gradient; an `NN_Ens` of 4 MLPs is trained twice on the same few points --
on the values alone (lam = 0) and with the reference's GradLoss penalty lam * mean((dM/dx - g)^2) -- and the error of the
surrogate's values and input gradients on held-out points is printed for both, followed by the posterior mean and standard
deviation of the input sensitivity dM/dx at a few points (`predict_jac_mom_sample`).
"""
import sys

import numpy as np
import torch

from quinn_amd.nns.mlp import MLP
from quinn_amd.solvers.nn_ens import NN_Ens


def model(x):
    y = (np.sin(x[:, 0]) * x[:, 1])[:, None]
    g = np.stack([np.cos(x[:, 0]) * x[:, 1], np.sin(x[:, 0])], axis=1)
    return y, g


def main(quick=False):
    torch.set_default_dtype(torch.double)
    ntrn, ntst = 20, 200
    xtrn = np.random.rand(ntrn, 2) * 4 - 2
    ytrn, gtrn = model(xtrn)
    xtst = np.random.rand(ntst, 2) * 4 - 2
    ytst, gtst = model(xtst)
    nnet = MLP(2, 1, (16, 16), biasorno=True, activ='tanh')
    nepochs = 100 if quick else 2000
    out = {}
    for lam in (0.0, 1.0):
        uqnet = NN_Ens(nnet, nens=4, dfrac=1.0, verbose=False)
        uqnet.fit(xtrn, ytrn, loss_fn='gradloss', gtrn=gtrn, lam=lam, lrate=0.01, batch_size=None, nepochs=nepochs)
        ypred = uqnet.predict_ens(xtst).mean(axis=0)
        jmean, jvar = uqnet.predict_jac_mom_sample(xtst, msc=1, nsam=4)
        rmse_y = float(np.sqrt(np.mean((ypred - ytst) ** 2)))
        rmse_g = float(np.sqrt(np.mean((jmean[:, 0, :] - gtst) ** 2)))
        print(f"lam = {lam}: test RMSE of the values {rmse_y:.4f}, of the input gradients {rmse_g:.4f}")
        out[lam] = (rmse_y, rmse_g, jmean, jvar)
    jmean, jvar = out[1.0][2:]
    print("input sensitivity dM/dx of the lam = 1 ensemble (mean +- std over the members) beside the truth:")
    for n in range(5):
        cells = "  ".join(f"d/dx{j}: {jmean[n, 0, j]:+.3f} +- {np.sqrt(jvar[n, 0, j]):.3f} ({gtst[n, j]:+.3f})" for j in range(2))
        print(f"  x = ({xtst[n, 0]:+.2f}, {xtst[n, 1]:+.2f})  {cells}")
    return out


if __name__ == '__main__':
    torch.manual_seed(0)
    np.random.seed(0)
    main(quick='--quick' in sys.argv)
