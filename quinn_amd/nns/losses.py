"""Losses: negative log-posterior and the derivative-informed `GradLoss`.

Mirror of the reference's `NegLogPost` (quinn/nns/losses.py:152-206):
    0.5*||y - f(x)||^2 / sigma^2 + (n/2) log 2 pi + n log sigma            (n = len(predictions))
  + n / fulldatasize * [ ||w - anchor||^2 / (2 sigma_p^2) + (K/2) log(2 pi sigma_p^2) ]   if priorparams
The data term comes from the batched HIP operator (sum of squared errors of the module's CURRENT
weights); the Gaussian prior term (`NegLogPrior`, losses.py:212-256) is an O(p) host formula.
"""
import numpy as np
import torch

from ..ops import MLPArch, BatchedMLP, flatten_module, neg_log_post_from_sse, check_gradloss_args


class NegLogPrior(torch.nn.Module):
    """Gaussian negative log-prior of a module's weights around an anchor (quinn/nns/losses.py:212-256):
    sum (w - anchor)^2 / (2 sigma^2) + (K/2) log(2 pi sigma^2).  O(p) host formula."""

    def __init__(self, sigma, anchor):
        super().__init__()
        self.sigma = float(sigma)
        self.anchor = anchor

    def forward(self, model):
        w = torch.cat([p.detach().flatten().double().cpu() for p in model.parameters()])
        a = torch.as_tensor(np.asarray(self.anchor.detach().cpu() if isinstance(self.anchor, torch.Tensor)
                                       else self.anchor), dtype=torch.float64).flatten()
        return ((w - a) ** 2).sum() / 2 / self.sigma ** 2 + (w.numel() / 2) * np.log(2 * np.pi * self.sigma ** 2)


class NegLogPost(torch.nn.Module):
    def __init__(self, nnmodel, fulldatasize, sigma, priorparams, device=None, dtype="float64"):
        super().__init__()
        self.nnmodel = nnmodel
        self.sigma = float(sigma)
        self.priorparams = priorparams
        self.fulldatasize = fulldatasize
        self._arch = MLPArch.from_module(nnmodel)
        self._opargs = dict(device=device, dtype=dtype)
        self._op = None

    def _operator(self, x, y):
        x = np.asarray(x.detach().cpu() if isinstance(x, torch.Tensor) else x, dtype=np.float64)
        y = np.asarray(y.detach().cpu() if isinstance(y, torch.Tensor) else y, dtype=np.float64)
        if self._op is None:
            self._op = BatchedMLP(self._arch, x, y.reshape(x.shape[0], -1), **self._opargs)
        else:
            self._op.set_data(x, y.reshape(x.shape[0], -1))
        return self._op

    def value_and_grad(self, weights, inputs, targets, want_grad=False):
        """(loss float, d loss / d weights (p,) or None) for one flat weight vector."""
        op = self._operator(inputs, targets)
        w = np.asarray(weights, dtype=np.float64).reshape(1, -1)
        n = op.N
        if want_grad:
            sse, g = op.sse_grad(w)
            grad = 0.5 * g[0].double().cpu().numpy() / self.sigma ** 2
        else:
            sse, grad = op.sse(w), None
        val = float(neg_log_post_from_sse(sse.cpu().numpy()[0], n, self.sigma))
        if self.priorparams is not None:
            sp = float(self.priorparams['sigma'])
            anchor = np.asarray(self.priorparams['anchor'].detach().cpu() if isinstance(
                self.priorparams['anchor'], torch.Tensor) else self.priorparams['anchor'], dtype=np.float64)
            K = w.shape[1]
            prior = np.sum((w[0] - anchor) ** 2) / 2 / sp ** 2 + (K / 2) * np.log(2 * np.pi * sp ** 2)
            val += n * prior / self.fulldatasize
            if want_grad:
                grad = grad + (n / self.fulldatasize) * (w[0] - anchor) / sp ** 2
        return val, grad

    def forward(self, inputs, targets):
        val, _ = self.value_and_grad(flatten_module(self.nnmodel), inputs, targets)
        return torch.tensor(val, dtype=torch.float64)


class GradLoss(torch.nn.Module):
    """Fit to function values AND observed input gradients (reference quinn/nns/losses.py:84-145):

        loss = mean((M(x) - y)^2) + lam * mean((dM/dx(xtrn) - gtrn)^2)

    Same constructor as the reference: nnmodel, lam, xtrn (N, d), gtrn (N, d) for one output or (N, o, d).  As there, the
    penalty is ALWAYS over the full `xtrn`, whatever minibatch `inputs` is:
        loss = sse(inputs) / (n_batch o) + lam gsse(xtrn) / (N o d).
    The reference's class cannot run as written -- its constructor stores `self._xtrn` / `self._gtrn` and `forward` reads
    `self.xtrn` / `self.gtrn` -- so no recorded result of it exists and the formula above is the contract.  Both sums and
    the weight gradient (a reverse pass over the forward-mode input Jacobian) come from the HIP kernels
    (`BatchedMLP.sobolev`); the reference loops `torch.autograd.functional.jacobian` over the rows."""

    def __init__(self, nnmodel, lam=0.0, xtrn=None, gtrn=None, device=None, dtype="float64"):
        super().__init__()
        self.nnmodel = nnmodel
        self.lam = float(lam)
        self._arch = MLPArch.from_module(nnmodel)
        if xtrn is None:
            raise ValueError("GradLoss needs xtrn, the points of the gradient observations")
        self.xtrn = np.asarray(xtrn.detach().cpu() if isinstance(xtrn, torch.Tensor) else xtrn, dtype=np.float64)
        self.xtrn = self.xtrn.reshape(-1, self._arch.dims[0])
        self.gtrn = check_gradloss_args(self._arch, dtype, self.xtrn, gtrn, self.lam)
        self._opargs = dict(device=device, dtype=dtype)
        self._op = self._opg = None

    def value_and_grad(self, weights, inputs, targets, want_grad=False):
        """(loss float, d loss / d weights (p,) or None) for one flat weight vector."""
        x = np.asarray(inputs.detach().cpu() if isinstance(inputs, torch.Tensor) else inputs, dtype=np.float64)
        y = np.asarray(targets.detach().cpu() if isinstance(targets, torch.Tensor) else targets, dtype=np.float64)
        d, o = self._arch.dims[0], self._arch.dims[-1]
        x = x.reshape(-1, d)
        nb, N = x.shape[0], self.xtrn.shape[0]
        if self._opg is None:                        # the penalty's operator: the gradient observations at xtrn
            self._opg = BatchedMLP(self._arch, self.xtrn, None, **self._opargs)
            self._opg.set_grad_data(self.gtrn)
            self._op = BatchedMLP(self._arch, x, y.reshape(nb, -1), **self._opargs)
            self._op.use_exact_float64()
        else:
            self._op.set_data(x, y.reshape(nb, -1))
        w = np.asarray(weights, dtype=np.float64).reshape(1, -1)
        cv, cg = 1.0 / (nb * o), self.lam / (N * o * d)
        _, gsse, gg = self._opg.sobolev(w, 0.0, cg, want_grad=want_grad)
        if want_grad:
            sse, gv = self._op.sse_grad(w)
            grad = (cv * gv[0].double() + gg[0]).cpu().numpy()
        else:
            sse, grad = self._op.sse(w), None
        return float(sse[0].item() * cv + gsse[0].item() * cg), grad

    def forward(self, inputs, targets):
        val, _ = self.value_and_grad(flatten_module(self.nnmodel), inputs, targets)
        return torch.tensor(val, dtype=torch.float64)
