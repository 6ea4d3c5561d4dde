"""Laplace approximation around per-member MAP fits.

Mirror of the reference's `NN_Laplace` (quinn/solvers/nn_laplace.py:11-154):
  1. MAP: every member minimises the negative log-posterior with a Gaussian prior around a random anchor on the rows
     `np.random.permutation(ntrn)[:int(ntrn*dfrac)]` -- exactly `NN_RMS.fit` (same batched run, same draw order).
  2. Curvature at the member's FINAL weights on its own rows, with the reference's `NegLogPost(model, ntrn, 0.1, None)`:
     the data noise is hard-wired to sigma = 0.1 there (a TODO of the reference) and there is no prior.
       'full':  H = (1/0.1^2) d2/dW2 sum_n |r_n|^2 / 2            (exact Hessian; may be indefinite)
       'diag':  H = diag( mean_n (d/dW |r_n|^2 / 2)^2 ) / 0.1^4     (empirical Fisher, dense (p,p) like the reference)
     One `qn_mlp_curv` call covers all members.  cov = inv(H * cov_scale) on the host (numpy), as the reference does.
     'ggn' / 'ggn_diag' (no counterpart in the reference): the generalised Gauss-Newton matrix G = sum_n sum_k J_nk^T J_nk of the
     member's rows (`qn_mlp_curv`, kinds GGN_FULL / GGN_DIAG) with the solver's OWN noise and prior,
       H = G / datanoise^2 + I / priorsigma^2,
     the Gauss-Newton Hessian of the objective the member minimised: positive definite by construction.  cov = inv(H * cov_scale)
     by a Cholesky factorisation on the device, where the covariance also stays for `predict_glm`.
  3. Prediction: `jens = np.random.randint(0, nens)`, then `np.random.multivariate_normal(means[jens], cov_mats[jens])`.
     The draws are replayed in that order with a per-member SVD factor computed once (numpy's own recipe, so the samples
     equal numpy's bit for bit); the M weight vectors then go through ONE batched device forward.
     'kron' (no counterpart in the reference): the Kronecker-factored Gauss-Newton.  Per Linear layer i two small matrices, the
     sums A_i = sum_n ~in_i ~in_i^T and S_i = sum_n sum_k g^k_i g^k_i^T over the member's Nb rows (`qn_mlp_kron_factors`, one
     call for all members); the layer block of G is approximated by (S_i (x) A_i) / Nb and cross-layer blocks by zero, so
       H_i = (S_i (x) A_i) / (Nb datanoise^2) + I / priorsigma^2
     is inverted EXACTLY through the two eigendecompositions (batched `torch.linalg.eigh` on the device; factor eigenvalues
     below 0 are clamped to 0): the variance of eigen-pair (a, c) is 1 / (cov_scale (l_S,a l_A,c / (Nb datanoise^2) +
     1 / priorsigma^2)).  No p x p array is formed -- the type for networks whose p is beyond 'ggn' (p > 16384).  Draws replay
     `np.random.randint`, then `np.random.standard_normal(p)` per sample, and are formed by ONE `qn_kron_sample` call;
     `predict_glm` goes through `qn_mlp_kron_glm_predict`.  `kron[j]` holds member j's factors, eigenbases and eigenvalues;
     `dense_cov(j)` materialises the covariance in flat parameter order for small networks.
  4. `predict_glm`: the linearised ("GLM") predictive in closed form -- one `qn_mlp_glm_predict` call gives every member's
     mean f_b(x_n) and output covariance J Sigma_b J^T; the members' Gaussians are mixed with equal weights.  No draws, no SVD.
"""
import warnings

import numpy as np
import torch

from .. import _lib, evidence, scoring
from ..ops import BatchedMLP, check_kron_args, kron_sample
from .nn_rms import NN_RMS

LA_SIGMA = 0.1          # nn_laplace.py:107: NegLogPost(learner.nnmodel, ntrn, 0.1, None)


def mvn_factor(cov):
    """(factor, psd) of numpy's legacy `multivariate_normal`: x = z @ (sqrt(s)[:, None] * v) + mean with
    (u, s, v) = svd(cov); psd is numpy's own check (allclose(v.T * s @ v, cov, rtol=atol=1e-8))."""
    cov = np.asarray(cov).astype(np.double)
    (_, s, v) = np.linalg.svd(cov)
    psd = np.allclose(np.dot(v.T * s, v), cov, rtol=1e-8, atol=1e-8)
    return np.sqrt(s)[:, None] * v, psd


def mvn_draw(mean, factor):
    """One draw of the global numpy generator, as `np.random.multivariate_normal(mean, cov)` makes it."""
    p = mean.shape[0]
    x = np.random.standard_normal([p]).reshape(-1, p)
    x = np.dot(x, factor)
    x += mean
    return x.reshape(p)


GGN_TYPES = ('ggn', 'ggn_diag')


def glm_mixture(f, S, noise_var=0.0):
    """Moments of the equal-weight mixture of M Gaussians N(f[b, n], S[b, n]) per query point (law of total variance):
    mean = avg_b f_b,  cov = avg_b (S_b + f_b f_b^T) - mean mean^T, plus noise_var on the diagonal.  noise_var `[M]` gives
    every member its own level: member b predicts N(f_b, S_b + noise_var_b I), which adds avg_b noise_var_b.
    f (M, N, o), S (M, N, o, o) -> (mean (N, o), cov (N, o, o)), numpy float64."""
    f = np.asarray(f, dtype=np.float64)
    S = np.asarray(S, dtype=np.float64)
    if np.ndim(noise_var) != 0:
        noise_var = np.asarray(noise_var, dtype=np.float64)
        if noise_var.shape != (f.shape[0],):
            raise ValueError(f"noise_var of shape {noise_var.shape}: one level, or one per member ({f.shape[0]})")
        noise_var = noise_var.mean()
    mean = f.mean(axis=0)
    second = (S + f[..., :, None] * f[..., None, :]).mean(axis=0)
    cov = second - mean[:, :, None] * mean[:, None, :]
    if noise_var:
        cov = cov + noise_var * np.eye(f.shape[-1])
    return mean, cov


class NN_Laplace(NN_RMS):
    """Args: nnmodel, la_type ('full' | 'diag' | 'ggn' | 'ggn_diag' | 'kron'), cov_scale, datanoise (of the MAP fit), priorsigma, and the
    `NN_Ens` keywords (nens, dfrac, verbose, device, dtype)."""

    def __init__(self, nnmodel, la_type='full', cov_scale=1.0, datanoise=0.1, priorsigma=1.0, **kwargs):
        super().__init__(nnmodel, datanoise=datanoise, priorsigma=priorsigma, **kwargs)
        self.la_type = la_type
        self.cov_scale = cov_scale
        self.means = []
        self.cov_mats = []
        self._factors = []
        self._cov_dev = []          # 'ggn': Sigma_j [p, p], 'ggn_diag': its diagonal [p], device float64 (None otherwise)
        self.kron = []              # 'kron': per member a dict of per-layer device tensors (see `_store_kron`)
        self._kron_packed = []      # 'kron': per member (UA [lenA], US [lenS], Dinv [p], Dih [p]) as the kernels take them
        self._kron_stack = None     # the members' packed tensors and means stacked (built on first use)
        self._G_dev = []            # 'ggn' / 'ggn_diag': the members' Gauss-Newton curvature G as the kernel returned it (device)
        self._ev_fit = None         # (xtrn, ytrn) of `fit`, and per `la_calc` member its (xtrn, ytrn): what the evidence's SSE needs
        self._ev_calc = []
        self._ev_cache = None       # (members, c [B, p], W [B, p], sse [B], n) of the evidence, built on its first call
        self._ev_logZ = None        # the members' log evidence at the scales in use (None: not computed yet)
        self.datanoise_ = None      # `tune_hyper(apply=True)`: the members' own noise levels [nens] ...
        self.prior_prec_ = None     # ... and prior precisions [nens, G] of the groups `prior_groups_`
        self.prior_groups_ = None

    def _kind(self):
        if self.la_type not in ('full', 'diag', 'kron') + GGN_TYPES:
            raise NotImplementedError(f"la_type {self.la_type!r}: only 'full', 'diag', 'ggn', 'ggn_diag' and 'kron' are accepted")
        return self.la_type

    def _store(self, w, hess):
        self.means.append(np.asarray(w, dtype=np.float64))
        self.cov_mats.append(np.linalg.inv(hess * self.cov_scale))
        self._factors.append(None)
        self._cov_dev.append(None)

    def _store_ggn(self, w, G):
        """One member of a GGN type from its device curvature G ([p, p] or [p]): H = G / datanoise^2 + I / priorsigma^2,
        cov = inv(H * cov_scale) by Cholesky on the device.  Returns H (numpy, dense)."""
        j = len(self.means)
        prior = 1.0 / self.priorsigma ** 2
        if self.la_type == 'ggn':
            H = G / self.datanoise ** 2
            H.diagonal().add_(prior)
            chol, info = torch.linalg.cholesky_ex(H * self.cov_scale)
            if int(info) != 0:
                raise np.linalg.LinAlgError(f"Cholesky factorisation of the Gauss-Newton Hessian of member {j} failed "
                                            f"(leading minor {int(info)} is not positive definite)")
            cov = torch.cholesky_inverse(chol)
            cov = 0.5 * (cov + cov.mT)
            cov_np = cov.cpu().numpy()
            H_np = H.cpu().numpy()
        else:
            h = G / self.datanoise ** 2 + prior
            if not bool(torch.all(h * self.cov_scale > 0)):
                raise np.linalg.LinAlgError(f"the diagonal Gauss-Newton Hessian of member {j} is not positive")
            cov = 1.0 / (h * self.cov_scale)
            cov_np = np.diag(cov.cpu().numpy())
            H_np = np.diag(h.cpu().numpy())
        self.means.append(np.asarray(w, dtype=np.float64))
        self.cov_mats.append(cov_np)
        self._factors.append(None)
        self._cov_dev.append(cov)
        self._G_dev.append(G)
        return H_np

    def _store_kron(self, W, A, S, lay, nb):
        """Members of type 'kron' from their factor sums A [B, lenA], S [B, lenS] (device) over nb rows each: batched
        eigendecompositions per layer, then the variances Dinv and standard deviations Dih of the eigen-pairs.  `kron[j]` gets
        nb, the layout and per-layer lists A, S (factors), UA, US (eigenvectors in the columns), lamA, lamS (eigenvalues,
        clamped at 0), Dinv [h_{i+1}, e_i]."""
        B = A.shape[0]
        prior = 1.0 / self.priorsigma ** 2
        scale = 1.0 / (nb * self.datanoise ** 2)
        UA, US = torch.empty_like(A), torch.empty_like(S)
        Dinv = torch.empty(B, lay.p, dtype=torch.float64, device=A.device)
        per = [dict(nb=nb, layout=lay, A=[], S=[], UA=[], US=[], lamA=[], lamS=[], Dinv=[]) for _ in range(B)]
        for i in range(len(lay.e)):
            Ai, Si = lay.A(A, i), lay.S(S, i)
            la_, ua = torch.linalg.eigh(Ai)
            ls_, us = torch.linalg.eigh(Si)
            la_, ls_ = la_.clamp_min(0.0), ls_.clamp_min(0.0)
            lay.A(UA, i).copy_(ua)
            lay.S(US, i).copy_(us)
            di = 1.0 / (self.cov_scale * (ls_[:, :, None] * la_[:, None, :] * scale + prior))
            lay.K(Dinv, i).copy_(di)
            for b in range(B):
                for key, v in (("A", Ai), ("S", Si), ("UA", ua), ("US", us), ("lamA", la_), ("lamS", ls_), ("Dinv", di)):
                    per[b][key].append(v[b])
        Dih = torch.sqrt(Dinv)
        for b in range(B):
            self.means.append(np.asarray(W[b], dtype=np.float64))
            self.cov_mats.append(None)
            self._factors.append(None)
            self._cov_dev.append(None)
            self.kron.append(per[b])
            self._kron_packed.append((UA[b], US[b], Dinv[b], Dih[b]))
        self._kron_stack = None

    def _kron_dev(self):
        """(means [B, p], UA, US, Dinv, Dih) of all members, stacked device tensors."""
        if self._kron_stack is None:
            dev = self._kron_packed[0][0].device
            mean = torch.as_tensor(np.asarray(self.means), device=dev).contiguous()
            self._kron_stack = (mean,) + tuple(torch.stack([m[q] for m in self._kron_packed]).contiguous() for q in range(4))
        return self._kron_stack

    def _kron_op(self, device):
        """The operator whose descriptor and layout `kron_sample` reuses (no data rows needed)."""
        if getattr(self, "_kron_sample_op", None) is None:
            self._kron_sample_op = BatchedMLP(self.arch, np.zeros((1, self.arch.dims[0])), None, device=device)
        return self._kron_sample_op

    def dense_cov(self, j):
        """Member j's covariance [p, p] in flat parameter order (numpy).  'kron': assembled from the eigen form, block by
        block -- for tests and small networks, refused for p > 16384; the other types return `cov_mats[j]`."""
        if self.la_type != 'kron':
            return self.cov_mats[j]
        k = self.kron[j]
        lay = k["layout"]
        if lay.p > 16384:
            raise ValueError(f"dense_cov is refused for p = {lay.p} > 16384 parameters ({lay.p ** 2 * 8e-9:.1f} GB)")
        cov = torch.zeros(lay.p, lay.p, dtype=torch.float64, device=k["UA"][0].device)
        perm = torch.as_tensor(lay.perm, device=cov.device)
        for i in range(len(lay.e)):
            Q = torch.kron(k["US"][i].contiguous(), k["UA"][i].contiguous())          # row (a, b), column (a', c)
            blk = (Q * k["Dinv"][i].reshape(-1)) @ Q.T
            idx = perm[lay.offK[i]:lay.offK[i] + lay.h[i] * lay.e[i]]
            cov[idx[:, None], idx[None, :]] = 0.5 * (blk + blk.T)
        return cov.cpu().numpy()

    def _scaled(self, curv):
        """Reference scaling of the kernels' result (numpy, one member)."""
        if self.la_type == 'full':
            return curv / LA_SIGMA ** 2
        return np.diag(curv / LA_SIGMA ** 4)

    def fit(self, xtrn, ytrn, **kwargs):
        """MAP fit of every member (`NN_RMS.fit`), then the curvature of all members in one batched call."""
        kind = self._kind()
        if kind == 'kron':
            check_kron_args(self.arch, self._dtype)
        super().fit(xtrn, ytrn, **kwargs)
        W = np.asarray(self.fit_results['final_w'], dtype=np.float64)
        self._ev_fit = (np.asarray(xtrn, dtype=np.float64), np.asarray(ytrn, dtype=np.float64).reshape(len(xtrn), -1))
        op = BatchedMLP(self.arch, self._ev_fit[0], self._ev_fit[1], device=self._device)
        if kind == 'kron':
            A, S, lay = op.kron_factors(W, row_idx=self.rows)
            self._store_kron(W, A, S, lay, np.asarray(self.rows).reshape(len(W), -1).shape[1])
            return
        if kind in GGN_TYPES:
            G = op.curvature(W, kind, row_idx=self.rows)
            self.hessians = [self._store_ggn(W[j], G[j]) for j in range(self.nens)]
            return
        curv = op.curvature(W, kind, row_idx=self.rows).cpu().numpy()
        self.hessians = [self._scaled(c) for c in curv]
        for j in range(self.nens):
            self._store(W[j], self.hessians[j])

    def la_calc(self, learner, xtrn, ytrn, batch_size=None):
        """Append the MAP centre and covariance of one learner (nn_laplace.py:76-122): Hessian at the learner's current
        weights on (xtrn, ytrn); with `batch_size` the sum of the per-batch results, as the reference forms it."""
        kind = self._kind()
        from ..ops import flatten_module
        w = flatten_module(learner.nnmodel)
        xtrn = np.asarray(xtrn, dtype=np.float64).reshape(len(xtrn), -1)
        ytrn = np.asarray(ytrn, dtype=np.float64).reshape(len(xtrn), -1)
        ntrn = len(xtrn)
        self._ev_calc.append((xtrn, ytrn))
        op = BatchedMLP(self.arch, xtrn, ytrn, device=self._device)
        if kind == 'kron':                      # factor sums add over the batches; the single 1 / Nb uses the total row count
            check_kron_args(self.arch, self._dtype)
            if not batch_size:
                A, S, lay = op.kron_factors(w[None])
            else:
                A = S = None
                for i in range(0, ntrn, batch_size):
                    rows = np.arange(i, min(ntrn, i + batch_size), dtype=np.int32)[None]
                    a, s_, lay = op.kron_factors(w[None], row_idx=rows)
                    A, S = (a, s_) if A is None else (A + a, S + s_)
            self._store_kron(w[None], A, S, lay, ntrn)
            return self.kron[-1]
        if kind in GGN_TYPES:                   # the prior enters once, after the per-batch Gauss-Newton sums
            if not batch_size:
                G = op.curvature(w[None], kind)[0]
            else:
                G = None
                for i in range(0, ntrn, batch_size):
                    rows = np.arange(i, min(ntrn, i + batch_size), dtype=np.int32)[None]
                    cur = op.curvature(w[None], kind, row_idx=rows)[0]
                    G = cur if G is None else G + cur
            return self._store_ggn(w, G)
        if not batch_size:
            hess = self._scaled(op.curvature(w[None], kind)[0].cpu().numpy())
        else:
            hess = None
            for i in range(ntrn // batch_size + 1):
                j = min(batch_size, ntrn - i * batch_size)
                if j > 0:
                    rows = np.arange(i * batch_size, i * batch_size + j, dtype=np.int32)[None]
                    cur = self._scaled(op.curvature(w[None], kind, row_idx=rows)[0].cpu().numpy())
                    hess = cur if i == 0 else hess + cur
        self._store(w, hess)
        return hess

    # -- prediction ------------------------------------------------------------------------------
    def _factor(self, j):
        if self._factors[j] is None:
            f, psd = mvn_factor(self.cov_mats[j])
            if not psd:
                warnings.warn(f"covariance of member {j} is not symmetric positive-semidefinite.", RuntimeWarning)
            self._factors[j] = f
        return self._factors[j]

    def _draw_weights(self, nens):
        """[M, p]: the reference's draws in its order (randint, then the member's multivariate normal) per sample."""
        if self.la_type == 'kron':
            js, Z = np.empty(nens, dtype=np.int32), np.empty((nens, self.nparams))
            for s in range(nens):
                js[s] = np.random.randint(0, self.nens)
                Z[s] = np.random.standard_normal(self.nparams)
            mean, UA, US, _, Dih = self._kron_dev()
            return kron_sample(self.arch, mean, UA, US, Dih, js, Z, op=self._kron_op(mean.device))
        W = np.empty((nens, self.nparams))
        for s in range(nens):
            jens = np.random.randint(0, self.nens)
            W[s] = mvn_draw(self.means[jens], self._factor(jens))
        return W

    def predict_sample(self, x):
        return self._predict_batch(self._draw_weights(1), x)[0]

    def _ens_weights(self, nens=1):
        return self._draw_weights(1 if nens is None else nens)

    def _predict_ens_dev(self, x, nens=1):
        return self._predict_batch_dev(self._ens_weights(nens), x)

    def predict_ens(self, x, nens=1):
        """`(M,N,o)`: M draws of `predict_sample` (nn_laplace.py:141-154), evaluated as one batched forward."""
        return self._predict_ens_dev(x, nens).double().cpu().numpy()

    def predict_ens_fromsamples(self, x, nens=1):
        return self.predict_ens(x, nens=nens)

    # -- linearised predictive -------------------------------------------------------------------
    def _glm_members(self, x):
        """The members' linearised predictives at x: (f [M, N, o] = f_b(x_n), S [M, N, o, o] = J_n Sigma_b J_n^T), float64
        device tensors, from one `qn_mlp_glm_predict` call ('kron': `qn_mlp_kron_glm_predict`)."""
        if not self.means:
            raise RuntimeError("the linearised predictive needs a fitted solver (fit or la_calc)")
        x = np.asarray(x, dtype=np.float64).reshape(len(x), -1)
        op = BatchedMLP(self.arch, x, None, device=self._device)
        if self.la_type == 'kron':
            mean, UA, US, Dinv, _ = self._kron_dev()
            f, S = op.kron_glm_predict(mean, UA, US, Dinv)
        else:
            diag = self.la_type in ('diag', 'ggn_diag')
            sig = []
            for j in range(len(self.means)):
                c = self._cov_dev[j]
                if c is None:
                    c = np.diag(self.cov_mats[j]) if diag else self.cov_mats[j]
                    c = torch.as_tensor(np.ascontiguousarray(c), device=op.device)
                sig.append(c)
            f, S = op.glm_predict(np.asarray(self.means), torch.stack(sig))
        return f, S

    def predict_glm(self, x, msc=1, noise=False):
        """Closed-form predictive of the network linearised at each member's MAP weights ("GLM" predictive):
        member b predicts N(f_b(x_n), J_n Sigma_b J_n^T) and the members are mixed with equal weights (`glm_mixture`).
        Returns (ymean (N,o), yvar (N,o) | None, ycov (N,o,o) | None); msc = 0 / 1 / 2 selects how much is returned.
        `ycov` is the covariance ACROSS THE OUTPUTS at each query point -- not `predict_mom_sample`'s (N,N,o), which is the
        covariance across the query points per output.  noise=True adds datanoise^2 to the (co)variance diagonal (after
        `tune_hyper(apply=True)`: every member's own tuned level).
        One `qn_mlp_glm_predict` call over all members ('kron': `qn_mlp_kron_glm_predict`, no p x p array); no weight draws and
        no SVD.  Works for every la_type; with 'full' the covariance may not be positive semi-definite, and negative variances
        are reported (warned about, not clipped)."""
        if msc not in (0, 1, 2):
            raise ValueError(f"msc={msc}, but needs to be 0, 1 or 2")
        if not self.means:
            raise RuntimeError("predict_glm needs a fitted solver (fit or la_calc)")
        f, S = self._glm_members(x)
        mean, cov = glm_mixture(f.cpu().numpy(), S.cpu().numpy(), self._member_noise_var() if noise else 0.0)
        var = np.stack([cov[:, k, k] for k in range(cov.shape[1])], axis=1)
        if np.any(var < 0):
            warnings.warn("predict_glm: negative predictive variance (the posterior covariance is not positive "
                          "semi-definite); values are not clipped.", RuntimeWarning)
        return mean, (var if msc >= 1 else None), (cov if msc == 2 else None)

    def score_glm(self, x, y, noise=None, crps=True, levels=scoring.DEFAULT_LEVELS, loo=False):
        """Score the closed-form linearised predictive against the targets y `(N, o)` at x: the dict of `QUiNNBase.score`, with
        member b predicting N(f_b(x_n)_k, noise^2 + (J_n Sigma_b J_n^T)_kk) per entry -- the members' means and the diagonal of
        their predictive covariances go to `qn_pred_score` as F and V.  No weight draws; `noise` defaults to `datanoise`
        (after `tune_hyper(apply=True)`: to every member's own tuned level, which then goes into V).
        With la_type 'full' a negative predictive variance makes that entry's scores NaN.  loo=True adds the PSIS-LOO keys, as
        in `QUiNNBase.score`."""
        own = noise is None and self.datanoise_ is not None
        sigma = 0.0 if own else self._score_noise(noise)
        y = np.asarray(y, dtype=np.float64).reshape(len(x), -1)
        f, S = self._glm_members(x)
        M = f.shape[0]
        V = torch.diagonal(S, dim1=-2, dim2=-1).contiguous()
        if own:
            V = V + torch.as_tensor(self.datanoise_ ** 2, device=V.device)[:, None, None]
        what = scoring.WHAT_ALL if crps else scoring.WHAT_ALL & ~_lib.SCORE_CRPS
        yt = torch.as_tensor(y.reshape(-1), device=f.device)
        F, V = f.contiguous().reshape(M, -1), V.reshape(M, -1)
        loo_rows = scoring.psis_rows(F, yt, sigma, V).cpu().numpy() if loo else None
        return scoring.summarise_all(scoring.score_rows(F, yt, sigma, V, what).cpu().numpy(), loo_rows, y, M, levels)

    def predict_glm_quantiles(self, x, q=(0.05, 0.5, 0.95), msc=1, noise=False):
        """`(Q, N, o)`: the quantiles at the levels q (0 < q < 1) of the closed-form linearised predictive of `predict_glm` --
        the equal-weight mixture of the members' Gaussians N(f_b(x_n)_k, (J_n Sigma_b J_n^T)_kk) per entry, with noise=True
        plus datanoise^2 (every member's own tuned level after `tune_hyper(apply=True)`).  The members' means and the diagonal
        of their predictive covariances go to `qn_pred_quantile` as F and V; no weight draws.  msc = 0 keeps the members'
        means only: the order-statistic quantiles of the f_b (levels in [0, 1]).  With la_type 'full' a variance that is not
        positive makes that entry NaN."""
        if msc not in (0, 1, 2):
            raise ValueError(f"msc={msc}, but needs to be 0, 1 or 2")
        f, S = self._glm_members(x)
        M, N, o = f.shape
        F = f.contiguous().reshape(M, -1)
        V = torch.diagonal(S, dim1=-2, dim2=-1).contiguous() if msc >= 1 else None
        if noise:
            nv = np.array(np.broadcast_to(np.asarray(self._member_noise_var(), dtype=np.float64), (M,)))
            nv = torch.as_tensor(nv, device=f.device)[:, None, None]
            V = nv.expand(M, N, o) if V is None else V + nv
        if V is not None:
            V = V.reshape(M, -1).contiguous()
        return scoring.quantile_rows(F, q, 0.0, V).cpu().numpy().reshape(-1, N, o)

    # -- evidence ---------------------------------------------------------------------------------
    def _member_noise_var(self):
        """datanoise^2, or the members' own `[M]` after `tune_hyper(apply=True)`."""
        return self.datanoise ** 2 if self.datanoise_ is None else self.datanoise_ ** 2

    def _evidence_inputs(self):
        """(c [B, p], W [B, p], sse [B], n) of all members, float64 device tensors: the curvature spectrum in units of G (see
        `quinn_amd.evidence`), the MAP weights in flat order and the SSE on the member's own rows -- ONE `BatchedMLP.sse` call
        for the members of `fit`, made on the first call and cached, like the spectrum."""
        evidence.check_groups(self._kind(), 'all')
        B = len(self.means)
        if B == 0:
            raise RuntimeError("the evidence needs a fitted solver (fit or la_calc)")
        if self._ev_cache is not None and self._ev_cache[0] == B:
            return self._ev_cache[1:]
        W = np.asarray(self.means)
        if self._ev_fit is not None and B == self.nens:
            op = BatchedMLP(self.arch, self._ev_fit[0], self._ev_fit[1], device=self._device)
            sse = op.sse(W, row_idx=self.rows)
            n = np.asarray(self.rows).reshape(B, -1).shape[1] * self._ev_fit[1].shape[1]
            dev = op.device
        elif len(self._ev_calc) == B:
            ns = {y.size for _, y in self._ev_calc}
            if len(ns) != 1:
                raise ValueError(f"the members of la_calc saw {sorted(ns)} entries of y: one evidence call needs the same n")
            ops = [BatchedMLP(self.arch, x, y, device=self._device) for x, y in self._ev_calc]
            sse = torch.cat([op.sse(W[j][None]) for j, op in enumerate(ops)])
            n, dev = ns.pop(), ops[0].device
        else:
            raise RuntimeError("the evidence needs the data of every member: members of `fit` and of `la_calc` are not mixed")
        if self.la_type == 'kron':
            c = torch.stack([evidence.kron_spectrum(k["lamS"], k["lamA"], k["nb"]) for k in self.kron])
        elif self.la_type == 'ggn_diag':
            c = torch.stack(self._G_dev)
        else:
            c = torch.linalg.eigvalsh(torch.stack(self._G_dev)).clamp_min(0.0)
        self._ev_cache = (B, c.contiguous(), torch.as_tensor(W, device=dev).contiguous(), sse.contiguous(), int(n))
        return self._ev_cache[1:]

    def _fit_scales(self):
        """(s2, tau) of the fit as float64 numpy scalars."""
        return np.float64(self.datanoise) ** 2, 1.0 / np.float64(self.priorsigma) ** 2

    def log_marginal_likelihood(self, datanoise=None, priorsigma=None, groups='all', full=False):
        """The Laplace approximation of every member's log marginal likelihood at its MAP weights (`quinn_amd.evidence`,
        `qn_la_evidence`): `[nens]` at the fit's own `datanoise` and `priorsigma`.  Over a grid -- datanoise `[Hc]` and / or
        priorsigma `[Hc]` or `[Hc, G]` (one scale per group of `groups`: 'all', 'layer', or 'tensor' for 'ggn_diag'), broadcast
        against each other; what is not given stays the fit's -- the result is `[nens, Hc]`.  full=True returns the dict of all
        rows: `logZ`, `loglik`, `logdet`, `gamma` (the effective number of parameters) and `gamma_g`, `S_g` `[..., G]`.
        la_type 'ggn', 'ggn_diag' and 'kron' ('ggn': groups='all' only; 'kron': not 'tensor').  `cov_scale` plays no part."""
        evidence.check_groups(self._kind(), groups)
        c, W, sse, n = self._evidence_inputs()
        bounds, _ = evidence.group_bounds(self.arch, groups)
        B, G = c.shape[0], len(bounds) - 1
        grid = np.ndim(datanoise) > 0 or np.ndim(priorsigma) > 0
        s2_fit, tau_fit = self._fit_scales()
        s2 = s2_fit if datanoise is None else np.asarray(datanoise, dtype=np.float64) ** 2
        tau = tau_fit if priorsigma is None else 1.0 / np.asarray(priorsigma, dtype=np.float64) ** 2
        if np.ndim(s2) > 1 or np.ndim(tau) > 2 or (np.ndim(tau) == 2 and tau.shape[1] != G):
            raise ValueError(f"datanoise is a scalar or [Hc], priorsigma a scalar, [Hc] or [Hc, {G}]")
        tau = np.asarray(tau)[..., None] if np.ndim(tau) < 2 else tau
        try:
            Hc = np.broadcast_shapes(np.shape(s2), tau.shape[:-1], (1,))[0]
        except ValueError:
            raise ValueError("datanoise and priorsigma do not broadcast against each other") from None
        s2 = np.ascontiguousarray(np.broadcast_to(s2, (B, Hc)))
        tau = np.ascontiguousarray(np.broadcast_to(tau, (B, Hc, G)))
        out = evidence.log_evidence_dev(c, W, sse, n, bounds, torch.as_tensor(s2, device=c.device),
                                        torch.as_tensor(tau, device=c.device)).cpu().numpy()
        if not grid:
            out = out[:, 0]
            if datanoise is None and priorsigma is None and self._ev_logZ is None:
                self._ev_logZ = out[:, 0].copy()
        if not full:
            return out[..., 0]
        no = len(evidence.ROWS)
        res = {name: out[..., i] for i, name in enumerate(evidence.ROWS)}
        res.update(gamma_g=out[..., no:no + G], S_g=out[..., no + G:])
        return res

    def tune_hyper(self, groups='layer', tol=evidence.DEFAULT_TOL, max_iter=evidence.DEFAULT_MAX_ITER, tune_noise=True,
                   tune_prior=True, apply=True):
        """Empirical Bayes, post hoc: every member's noise level and per-group prior precisions by maximising its Laplace evidence
        at its MAP weights (MacKay's fixed point, `quinn_amd.evidence.tune`), one `qn_la_tune` launch for all members, from the
        fit's scales.  Returns a dict: `datanoise` `[nens]`, `prior_prec` `[nens, G]`, `prior_groups` (the groups' names),
        `logZ`, `logZ_start`, `gamma` `[nens, G]`, `iters`, `converged`, `clamped` (the OR of the `evidence.CLAMP_` bits), `resid`.
        A member that did not converge within max_iter returns the best iterate seen, so logZ >= logZ_start always.
        apply=True rebuilds every member's posterior at its own tuned scales ('kron', 'ggn_diag': the variances come from the
        same launch; 'ggn': one device Cholesky per member); `predict_ens`, `predict_glm` and `score_glm` then use them, and
        their noise default becomes each member's own level.  The tuned values are kept in `datanoise_` / `prior_prec_`;
        `datanoise` / `priorsigma` stay the fit's.  The MAP weights are not refitted."""
        evidence.check_groups(self._kind(), groups)
        c, W, sse, n = self._evidence_inputs()
        bounds, names = evidence.group_bounds(self.arch, groups)
        B, G = c.shape[0], len(bounds) - 1
        s2_fit, tau_fit = self._fit_scales()
        s2_0 = torch.full((B,), float(s2_fit), dtype=torch.float64, device=c.device)
        tau_0 = torch.full((B, G), float(tau_fit), dtype=torch.float64, device=c.device)
        want = bool(apply) and self.la_type in ('kron', 'ggn_diag')
        dev = evidence.tune_dev(c, W, sse, n, bounds, s2_0, tau_0, tol=tol, max_iter=max_iter, tune_noise=tune_noise,
                                tune_prior=tune_prior, cov_scale=self.cov_scale, want_dinv=want)
        s2, tau, rows, status = (dev[k].cpu().numpy() for k in ("s2", "tau", "rows", "status"))
        no = len(evidence.ROWS)
        res = dict(datanoise=np.sqrt(s2), prior_prec=tau, prior_groups=list(names), logZ=rows[:, 0], logZ_start=status[:, 4],
                   gamma=rows[:, no:no + G], iters=status[:, 0].astype(np.int64), converged=status[:, 2].astype(bool),
                   clamped=status[:, 5].astype(np.int64), resid=status[:, 3])
        if not apply:
            return res
        if np.any(np.isnan(rows[:, 0])):
            raise np.linalg.LinAlgError("tune_hyper: the evidence of a member is NaN (a non-finite weight, curvature or SSE); "
                                        "nothing was applied")
        if self.la_type == 'kron':
            for j in range(B):
                UA, US = self._kron_packed[j][:2]
                self._kron_packed[j] = (UA, US, dev["Dinv"][j], dev["Dih"][j])
                lay = self.kron[j]["layout"]
                self.kron[j]["Dinv"] = [lay.K(dev["Dinv"][j], i) for i in range(len(lay.e))]
            self._kron_stack = None
        elif self.la_type == 'ggn_diag':
            for j in range(B):
                self._cov_dev[j] = dev["Dinv"][j]
                self.cov_mats[j] = np.diag(dev["Dinv"][j].cpu().numpy())
                self._factors[j] = None
        else:
            for j in range(B):
                H = self._G_dev[j] / dev["s2"][j]
                H.diagonal().add_(dev["tau"][j, 0])
                chol, info = torch.linalg.cholesky_ex(H * self.cov_scale)
                if int(info) != 0:
                    raise np.linalg.LinAlgError(f"Cholesky factorisation of the tuned Gauss-Newton Hessian of member {j} failed")
                cov = torch.cholesky_inverse(chol)
                cov = 0.5 * (cov + cov.mT)
                self._cov_dev[j], self.cov_mats[j], self._factors[j] = cov, cov.cpu().numpy(), None
        self.datanoise_, self.prior_prec_, self.prior_groups_ = res["datanoise"].copy(), tau.copy(), list(names)
        self._ev_logZ = res["logZ"].copy()
        return res

    def evidence_weights(self):
        """`[nens]`: the softmax of the members' log evidence (numpy) at the scales in use -- the tuned ones after
        `tune_hyper(apply=True)`, else the fit's -- for `score(..., member_weights=)` of one draw per member in member order."""
        if self._ev_logZ is None:
            self.log_marginal_likelihood()
        return evidence.softmax_weights(self._ev_logZ)
