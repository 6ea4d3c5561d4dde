"""SWAG (Stochastic Weight Averaging Gaussian) around per-member MAP fits.

Mirror of the reference's `NN_SWAG` (quinn/solvers/nn_swag.py):
  1. MAP: every member minimises the negative log-posterior WITHOUT prior (the reference's `priorparams` line is commented
     out, so `priorsigma` is stored and never used) on the rows `np.random.permutation(ntrn)[:int(ntrn*dfrac)]` -- the
     batched `fit_members` run of `NN_Ens.fit` with loss_fn='logpost'.
  2. SWAG phase from the member's FINAL MAP weights, on its own rows: n_steps full-batch SGD steps of the reference's default
     loss (MSE, mean over rows and outputs), learning rate lr_swag, no weight decay.  Every c-th step the running moments
     m1, m2 and (lowrank) the deviation w - m1 (of the updated mean) are collected; the last k deviations are kept.
     Per step, for all members at once: one `sse_grad` and one fused `qn_swag_step`.
  3. Prediction: `jens = randint(0, nens)`, `z1 = randn(nparams)`, `z2 = randn(k)` per draw, replayed on the host in the
     reference's order; one `qn_swag_sample` forms every theta, one batched forward evaluates them.  The reference adds
     the correction to `means[jens]` IN PLACE (`theta = self.means[jens]; theta += ...`), so every draw moves the stored
     mean of its member; `mean_drift=True` (default) keeps that, `mean_drift=False` samples around the collected mean as
     the SWAG paper describes.

Torch's generator: member j draws its nepochs MAP permutations and then its n_steps SWAG permutations before member j+1
draws (`draw_perms(nens, nepochs + n_steps, nsub)` split at nepochs).  The moments live on the device; `means`,
`cov_diags` and `d_mats` are numpy views of them in the reference's shapes (`d_mats[j]` is (p, k), oldest column first).
"""
import numpy as np
import torch

from .. import _lib
from ..nns.nnfit import fit_members, load_flat_into, draw_perms
from ..ops import BatchedMLP, check_swag_args, flatten_module, swag_sample, swag_step
from ..parallel import shard_bounds, all_gather_rows, dist_info
from .nn_ens import NN_Ens


class NN_SWAG(NN_Ens):
    """Args: nnmodel, k (deviation columns), n_steps (SGD steps of the SWAG phase), c (collection period), cov_type
    ('lowrank'; anything else: diagonal), lr_swag, datanoise (of the MAP fit), priorsigma (unused, as in the reference),
    mean_drift (see the module docstring) and the `NN_Ens` keywords (nens, dfrac, verbose, device, dtype)."""

    def __init__(self, nnmodel, k=10, n_steps=12, c=1, cov_type="lowrank", lr_swag=0.1, datanoise=0.1, priorsigma=1.0,
                 mean_drift=True, **kwargs):
        self._lowrank = check_swag_args(k, n_steps, c, cov_type)
        super().__init__(nnmodel, **kwargs)
        self.k, self.n_steps, self.c, self.cov_type = k, n_steps, c, cov_type
        self.lr_swag = lr_swag
        self.datanoise = datanoise
        self.priorsigma = priorsigma
        self.mean_drift = bool(mean_drift)
        self.nparams = sum(p.numel() for p in self.nnmodel.parameters())
        self._mean_d = self._diag_d = self._D_d = None

    # -- the posterior, device-resident; numpy views in the reference's shapes --------------------------------------------
    @property
    def means(self):
        return [] if self._mean_d is None else list(self._mean_d.cpu().numpy())

    @property
    def cov_diags(self):
        return [] if self._diag_d is None else list(self._diag_d.cpu().numpy())

    @property
    def d_mats(self):
        return [] if self._D_d is None else [d.T.copy() for d in self._D_d.cpu().numpy()]

    def fit(self, xtrn, ytrn, **kwargs):
        """MAP fit of every member (one batched run), then the SWAG phase of every member in lock step."""
        ntrn = ytrn.shape[0]
        rows = np.stack([np.random.permutation(ntrn)[:int(ntrn * self.dfrac)] for _ in range(self.nens)])
        val = kwargs.pop('val', None)
        xval, yval = (None, None) if val is None else val      # None: members validate on their own rows
        for key in ('freq_plot', 'lhist_suffix', 'gradcheck', 'lossparams', 'loss_fn', 'datanoise'):
            kwargs.pop(key, None)
        if kwargs.pop('priorparams', None) is not None:
            raise NotImplementedError("the reference's SWAG MAP fit has no prior (use NN_RMS for one)")
        nepochs = kwargs.pop('nepochs', 5000)
        nsub = rows.shape[1]
        lo, hi = shard_bounds(self.nens)
        perms = None
        if kwargs.get('perm_mode', 'reference') == 'reference':
            perms = draw_perms(self.nens, nepochs + self.n_steps, nsub)[lo:hi]
        w0 = flatten_module(self.learners[0].nnmodel)
        verbose = self.verbose and dist_info()[0] == 0
        res = fit_members(self.arch, np.tile(w0, (hi - lo, 1)), xtrn, ytrn, rows[lo:hi], xval, yval, nepochs,
                          kwargs.pop('batch_size', None), loss_fn='logpost', datanoise=self.datanoise,
                          device=self._device, dtype=self._dtype, verbose=verbose,
                          perms=None if perms is None else np.ascontiguousarray(perms[:, :nepochs]), **kwargs)
        W_map = res['final_w']
        res = {key: all_gather_rows(v, self.nens) for key, v in res.items()}
        self.fit_results, self._best_w, self.rows = res, res['best_w'], rows
        for j, learner in enumerate(self.learners):
            learner._best_model, learner._best_w, learner._pred_op = None, res['best_w'][j], None
            learner.history = [list(r) for r in res['history'][j]]
            learner.trained = True
        W, m1, m2, D = self._swag_phase(W_map, xtrn, ytrn, rows[lo:hi],
                                        None if perms is None else perms[:, nepochs:])
        ncol = self.n_steps // self.c
        if D is not None:                                        # ring buffer -> columns oldest to newest
            order = torch.tensor([(ncol + t) % self.k for t in range(self.k)], device=D.device)
            D = D.index_select(1, order)
        diag = m2 - m1 * m1                                     # moment2 - moment1**2 (two roundings, as numpy)
        W_fin = W.cpu().numpy()
        if dist_info()[1] > 1:                                   # members shard over ranks: every rank gets all of them
            dev = m1.device
            m1, diag = (torch.as_tensor(all_gather_rows(t, self.nens), device=dev) for t in (m1, diag))
            D = None if D is None else torch.as_tensor(all_gather_rows(D, self.nens), device=dev)
            W_fin = all_gather_rows(W_fin, self.nens)
        self._mean_d, self._diag_d, self._D_d = m1.contiguous(), diag.contiguous(), None if D is None else D.contiguous()
        for j, learner in enumerate(self.learners):              # the module ends at the last SWAG weights
            load_flat_into(learner.nnmodel, W_fin[j])

    def _swag_phase(self, W0, xtrn, ytrn, rows, perms):
        """swag_calc (nn_swag.py:86-123) for this rank's members: (W, m1, m2, D ring buffer or None), device float64."""
        xtrn = np.asarray(xtrn, dtype=np.float64).reshape(len(xtrn), -1)
        ytrn = np.asarray(ytrn, dtype=np.float64).reshape(len(xtrn), -1)
        op = BatchedMLP(self.arch, xtrn, ytrn, device=self._device, dtype=self._dtype)
        dev = op.device
        B, nsub, o = rows.shape[0], rows.shape[1], ytrn.shape[1]
        W = torch.as_tensor(np.ascontiguousarray(W0, dtype=np.float64), device=dev).reshape(B, self.nparams).clone()
        if B == 0:                                               # this rank owns no member
            D = torch.zeros(0, self.k, self.nparams, dtype=torch.float64, device=dev) if self._lowrank else None
            return W, W.clone(), W.clone(), D
        m1, m2 = torch.empty_like(W), torch.empty_like(W)
        D = torch.zeros(B, self.k, self.nparams, dtype=torch.float64, device=dev) if self._lowrank else None
        swag_step(_lib.SWAG_INIT, W, m1=m1, m2=m2)
        if self.n_steps == 0:
            return W, m1, m2, D
        rows_d = torch.as_tensor(rows, device=dev, dtype=torch.int64)
        if perms is not None:                                    # the step's permutation of the member's rows
            idx = torch.gather(rows_d[:, None, :].expand(B, self.n_steps, nsub), 2,
                               torch.as_tensor(np.ascontiguousarray(perms), device=dev)).to(torch.int32).contiguous()
        else:
            idx = rows_d.to(torch.int32)[:, None, :].expand(B, self.n_steps, nsub).contiguous()
        lr = torch.full((B,), float(self.lr_swag), dtype=torch.float64, device=dev)
        sse = torch.empty(B, dtype=torch.float64, device=dev)
        G = torch.empty(B, self.nparams, dtype=op.tdt, device=dev)
        gscale = 1.0 / (nsub * o)                                # MSELoss(reduction='mean') of nnfit's default loss
        Wc = W if op.tdt == torch.float64 else torch.empty(B, self.nparams, dtype=op.tdt, device=dev)
        for i in range(1, self.n_steps + 1):
            if Wc is not W:
                Wc.copy_(W)
            op.sse_grad(Wc, row_idx=idx[:, i - 1], out=(sse, G))
            if i % self.c == 0:
                n = i // self.c
                swag_step(_lib.SWAG_SGD_COLLECT, W, G, lr, gscale, m1, m2, D, slot=(n - 1) % self.k, n=n)
            else:
                swag_step(_lib.SWAG_SGD, W, G, lr, gscale)
        return W, m1, m2, D

    # -- prediction ------------------------------------------------------------------------------
    def _draws(self, nens):
        """The reference's numpy draws for `nens` predict_sample calls, in its order: (js [M], z1 [M, p], z2 [M, k])."""
        js = np.empty(nens, dtype=np.int64)
        z1 = np.empty((nens, self.nparams))
        z2 = np.empty((nens, self.k))
        for s in range(nens):
            js[s] = np.random.randint(0, self.nens)
            z1[s] = np.random.randn(self.nparams)
            z2[s] = np.random.randn(self.k)                     # drawn for the diagonal covariance too
        return js, z1, z2

    def sample_weights(self, nens=1):
        """[M, p] float64 device tensor of M posterior draws (moves the means when mean_drift is set)."""
        if self._mean_d is None:
            raise RuntimeError("NN_SWAG: fit() first")
        js, z1, z2 = self._draws(nens)
        return swag_sample(self._mean_d, self._diag_d, self._D_d, js, z1, z2, self.mean_drift)

    def predict_sample(self, x):
        return self._predict_batch(self.sample_weights(1), x)[0]

    def _ens_weights(self, nens=1):
        return self.sample_weights(1 if nens is None else nens)

    def _predict_ens_dev(self, x, nens=1):
        return self._predict_batch_dev(self._ens_weights(nens), x)

    def predict_ens(self, x, nens=1):
        """`(M,N,o)`: M draws of `predict_sample` (nn_swag.py:147-160), evaluated as one batched forward."""
        return self._predict_ens_dev(x, nens).double().cpu().numpy()

    def predict_ens_fromsamples(self, x, nens=1):
        return self.predict_ens(x, nens=nens)
