#!/usr/bin/env python
"""Score three posteriors of one small regression side by side on held-out rows: device HMC, a deep ensemble and a
Kronecker-factored Laplace approximation (its weight draws and its closed-form linearised predictive).

`score` draws the solver's predictive ensemble once and reduces it on the device to lppd / WAIC, PIT coverage and the
CRPS (`quinn_amd.scoring`); lower nlpd and crps are better, and coverage[0.9] should be near 0.9.  On the training rows
`loo=True` adds PSIS-LOO: `elpd_loo` estimates what `elpd_waic` does, and `n_khat_bad` counts the rows on which the
importance weights are too heavy-tailed for either to be trusted."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from quinn_amd.nns.mlp import MLP                                # noqa: E402
from quinn_amd.solvers.nn_ens import NN_Ens                      # noqa: E402
from quinn_amd.solvers.nn_laplace import NN_Laplace              # noqa: E402
from quinn_amd.solvers.nn_mcmc import NN_MCMC                    # noqa: E402

NOISE = 0.1


def line(name, s):
    cov = "  ".join(f"cov{int(100 * k)}={v:.2f}" for k, v in s["coverage"].items())
    print(f"{name:<22} nlpd={s['nlpd']:8.3f}  crps={s['crps']:.4f}  rmse={s['rmse']:.4f}  p_waic={s['p_waic']:8.2f}  {cov}")


def loo_line(name, s):
    print(f"{name:<22} elpd_waic={s['elpd_waic']:9.2f}  elpd_loo={s['elpd_loo']:9.2f}  p_loo={s['p_loo']:7.2f}  "
          f"n_khat_bad={s['n_khat_bad']}/{s['n']} (khat > {s['khat_threshold']:.2f})")


def main():
    torch.manual_seed(0)
    np.random.seed(0)
    rs = np.random.RandomState(0)
    x = rs.rand(104, 1) * 6 - 3
    y = np.sin(x) + NOISE * rs.randn(104, 1)
    xtrn, ytrn, xtst, ytst = x[:64], y[:64], x[64:], y[64:]
    net = MLP(1, 1, (11, 11), biasorno=True, activ='tanh').double()

    hmc = NN_MCMC(net, verbose=False)
    ini = np.stack([np.random.RandomState(100 + c).rand(hmc.pdim) * 0.2 for c in range(4)])
    hmc.fit(xtrn, ytrn, zflag=False, datanoise=NOISE, nmcmc=400, param_ini=ini, sampler='hmc',
            sampler_params={'epsilon': 2e-3, 'L': 5, 'adapt': 150}, nchains=4, seeds=list(range(4)), engine='device')
    line("HMC (4 chains)", hmc.score(xtst, ytst, nsam=100, nburn=200, chain='all'))

    ens = NN_Ens(net, nens=8, dfrac=0.8, verbose=False)
    ens.fit(xtrn, ytrn, lrate=0.01, batch_size=16, nepochs=200, freq_out=1000)
    line("deep ensemble (8)", ens.score(xtst, ytst, noise=NOISE))

    la = NN_Laplace(net, la_type='kron', nens=2, dfrac=0.8, datanoise=NOISE, verbose=False)
    la.fit(xtrn, ytrn, val=[xtst, ytst], lrate=0.01, batch_size=16, nepochs=200, freq_out=1000)
    line("Laplace kron, draws", la.score(xtst, ytst, nsam=100))
    line("Laplace kron, score_glm", la.score_glm(xtst, ytst))
    line("HMC on training (WAIC)", hmc.score(xtrn, ytrn, nsam=100, nburn=200, chain='all'))
    print("training rows, WAIC beside PSIS-LOO:")
    loo_line("HMC (4 chains)", hmc.score(xtrn, ytrn, nsam=100, nburn=200, chain='all', loo=True))
    loo_line("deep ensemble (8)", ens.score(xtrn, ytrn, noise=NOISE, loo=True))
    loo_line("Laplace kron, draws", la.score(xtrn, ytrn, nsam=100, loo=True))


if __name__ == "__main__":
    main()
