"""Base class of the probabilistic wrappers.

Mirror of the reference's `QUiNNBase` (quinn/solvers/quinn.py:15-104): deep-copies the user
module, `predict_ens` stacks `predict_sample` draws, `predict_mom_sample` forms mean /
variance / covariance over that ensemble.  The matplotlib helpers of the reference
(`predict_plot`, `plot_1d_fits`, quinn.py:106-251) are presentation code outside the hot
path and are not reproduced.
"""
import copy
import sys

import numpy as np
import torch

from .. import _lib, scoring
from ..ops import MLPArch, BatchedMLP, flatten_module


def print_nnparams(nnmodel, names_only=False):
    for name, param in nnmodel.named_parameters():
        if names_only:
            print(f"{name}, shape {tuple(param.data.shape)}")
        else:
            print(name, param.data)


class QUiNNBase():
    """Args: nnmodel (torch.nn.Module): the user's MLP (never modified in place)."""

    def __init__(self, nnmodel, device=None, dtype="float64"):
        self.nnmodel = copy.deepcopy(nnmodel)
        self.nens = None
        self.arch = MLPArch.from_module(self.nnmodel)
        self._device = device
        self._dtype = dtype
        self._pred_op = None

    def print_params(self, names_only=False):
        print_nnparams(self.nnmodel, names_only=names_only)

    # -- device operator used for predictions (dataset = the query points) --------------
    def _predict_batch_dev(self, W, x):
        """f_W(x) for a stack of flat weight vectors: device tensor (M, N, o) in the compute dtype."""
        x = np.asarray(x, dtype=np.float64)
        if self._pred_op is None:
            self._pred_op = BatchedMLP(self.arch, x, None, device=self._device, dtype=self._dtype)
        return self._pred_op.predict(W, x)

    def _predict_batch(self, W, x):
        """f_W(x) for a stack of flat weight vectors: numpy (M, N, o)."""
        return self._predict_batch_dev(W, x).double().cpu().numpy()

    def predict_sample(self, x):
        raise NotImplementedError

    def _predict_ens_dev(self, x, nens):
        """The predictive ensemble as a DEVICE tensor (M, N, o).  Solvers whose members come out of one batched forward
        override this (no host round trip); the default takes whatever `predict_ens` of the solver returns."""
        return torch.as_tensor(self.predict_ens(x, nens=nens))

    def predict_ens(self, x, nens=None):
        """`(M, N, o)`: M draws of `predict_sample` (quinn.py:51-70)."""
        if nens is None:
            nens = self.nens
        return np.array([self.predict_sample(x) for _ in range(nens)])

    def predict(self, x):
        return self.predict_mom_sample(x)[0]

    def predict_mom_sample(self, x, msc=0, nsam=1000, **ens_args):
        """Mean `(N,o)`, variance `(N,o)` (ddof=1) and per-output covariance `(N,N,o)` of an
        `nsam`-member predictive ensemble; msc = 0 / 1 / 2 selects how much is computed
        (quinn.py:75-104).  The ensemble stays on the device: mean / variance by `qn_pred_moments`, the
        covariance as one float64 GEMM of the centred ensemble per output; only the moments are downloaded.
        ens_args go to the solver's ensemble (NN_MCMC: `nburn`, `chain`, e.g. chain='all' pools the chains)."""
        if msc not in (0, 1, 2):
            print(f"msc={msc}, but needs to be 0,1, or 2. Exiting.")
            sys.exit()
        dev = torch.device(self._device) if self._device is not None else torch.device("cuda", torch.cuda.current_device())
        y = self._predict_ens_dev(x, nsam, **ens_args).to(dev).contiguous()
        M, nx, nout = y.shape
        mean = torch.empty(nx, nout, dtype=torch.float64, device=dev)
        var = torch.empty(nx, nout, dtype=torch.float64, device=dev) if msc == 1 else None
        qdt = _lib.QN_F32 if y.dtype == torch.float32 else _lib.QN_F64
        if y.dtype not in (torch.float32, torch.float64):
            y, qdt = y.double(), _lib.QN_F64
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().qn_pred_moments(y.data_ptr(), qdt, M, nx * nout, mean.data_ptr(),
                                                  var.data_ptr() if var is not None else None,
                                                  _lib.stream(dev)), "qn_pred_moments")
        ymean = mean.cpu().numpy()
        if msc == 2:
            yc = y.double() - mean                                   # (M, N, o)
            ycov_d = torch.empty(nx, nx, nout, dtype=torch.float64, device=dev)
            for iout in range(nout):
                a = yc[:, :, iout]
                ycov_d[:, :, iout] = (a.T @ a) / (M - 1)            # np.cov(rowvar=False, ddof=1), quinn.py:88-90
            ycov = ycov_d.cpu().numpy()
            yvar = np.stack([np.diag(ycov[:, :, iout]) for iout in range(nout)], axis=1)
        elif msc == 1:
            ycov, yvar = None, var.cpu().numpy()
        else:
            ycov, yvar = None, None
        return ymean, yvar, ycov

    # -- input sensitivities dM/dx under the posterior (qn_mlp_input_jac) ---------------------------------
    def _ens_weights(self, nens=None, **ens_args):
        """The flat weight vectors `(M, p)` (numpy or device tensor) behind the solver's predictive ensemble, drawn exactly as
        `predict_ens` draws them."""
        raise NotImplementedError(f"{type(self).__name__} does not expose the weights of its predictive ensemble")

    def _predict_jac_dev(self, x, nens=None, **ens_args):
        W = self._ens_weights(nens, **ens_args)
        x = np.asarray(x, dtype=np.float64)
        if self._dtype != "float64":
            raise ValueError(f"input sensitivities need the float64 operator (got dtype {self._dtype!r})")
        if getattr(self, "_jac_op", None) is None:
            self._jac_op = BatchedMLP(self.arch, x, None, device=self._device, dtype="float64")
        return self._jac_op.input_jacobian(W, x)

    def predict_jac_ens(self, x, nens=None, **ens_args):
        """`(M, N, o, d)`: the input Jacobian d f_k(x_n) / d x_j of every member of the solver's predictive ensemble (the
        members `predict_ens(x, nens, **ens_args)` evaluates), from one batched tangent forward."""
        return self._predict_jac_dev(x, nens, **ens_args).cpu().numpy()

    def predict_jac_mom_sample(self, x, msc=0, nsam=1000, **ens_args):
        """Mean `(N, o, d)` and, with msc = 1, variance `(N, o, d)` (ddof=1; else None) of the input sensitivity over an
        `nsam`-member posterior ensemble.  The Jacobians stay on the device; the moments come from `qn_pred_moments`."""
        if msc not in (0, 1):
            raise ValueError(f"msc={msc}, but needs to be 0 or 1")
        J = self._predict_jac_dev(x, nsam, **ens_args).contiguous()
        dev = J.device
        M, K = J.shape[0], J[0].numel()
        mean = torch.empty(J.shape[1:], dtype=torch.float64, device=dev)
        var = torch.empty(J.shape[1:], dtype=torch.float64, device=dev) if msc == 1 else None
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().qn_pred_moments(J.data_ptr(), _lib.QN_F64, M, K, mean.data_ptr(),
                                                  var.data_ptr() if var is not None else None,
                                                  _lib.stream(dev)), "qn_pred_moments")
        return mean.cpu().numpy(), (var.cpu().numpy() if var is not None else None)

    # -- scores of the predictive against data (qn_pred_score) ---------------------------------------------
    def _score_noise(self, noise):
        """The data noise sigma of the Gaussian predictive: `noise`, or the one the last fit used where the solver keeps it."""
        if noise is None:
            lpinfo = getattr(self, 'lpinfo', None)
            if lpinfo and 'sigma' in lpinfo.get('lparams', {}):
                noise = lpinfo['lparams']['sigma']
            else:
                noise = getattr(self, 'datanoise', None)
        if noise is None:
            raise ValueError(f"{type(self).__name__} keeps no data noise: pass noise=")
        return float(noise)

    def _score_member_noise(self, noise, nsam, **ens_args):
        """`(M,)` noise levels, one per member of the ensemble `_ens_weights(nsam, **ens_args)` draws, where the solver sampled
        the noise level and `noise` is None; else None (one level for all members: `_score_noise`)."""
        return None

    def _ens_weights_ordered(self, nens=None, **ens_args):
        """`_ens_weights` in an order that two calls reproduce, for per-member weights; a solver whose `_ens_weights` shuffles
        the members overrides this."""
        return self._ens_weights(nens, **ens_args)

    def _score_chunks(self, W, x, y, member, max_bytes):
        """(lo, hi, F `(M, rows * o)`, y chunk or None, V or None) over the row chunks of `score` (y `(N, o)` or None)."""
        M, N, o = len(W), len(x), (self.arch.dims[-1] if y is None else y.shape[1])
        esize = 4 if self._dtype == "float32" else 8
        step = max(1, int(max_bytes) // (M * o * esize))
        for lo in range(0, N, step):
            hi = min(N, lo + step)
            F = self._predict_batch_dev(W, x[lo:hi]).contiguous()
            if F.dtype not in (torch.float32, torch.float64):
                F = F.double()
            yt = None if y is None else torch.as_tensor(y[lo:hi].reshape(-1), device=F.device)
            F = F.reshape(M, -1)
            V = None if member is None else (torch.as_tensor(member, device=F.device) ** 2).to(F.dtype)[:, None].expand_as(F).contiguous()
            yield lo, hi, F, yt, V

    def _stack_groups(self, x, y, W, offsets, member, sigma, loo, tol, max_iter, max_bytes):
        """The stacking of the groups offsets[g] .. offsets[g + 1] - 1 of the weight vectors W `(M, p)` on the data (x, y): L
        `[G, N * o]` is assembled on the device over the row chunks of `score` (`scoring.group_lpd`), `scoring.stack_weights`
        optimises, and the dict documented at `NN_MCMC.stack` is stored as `self.stacking` and returned."""
        from .. import stacking
        x = np.asarray(x, dtype=np.float64).reshape(len(x), -1)
        y = np.asarray(y, dtype=np.float64).reshape(len(x), -1)
        N, o = y.shape
        G = len(offsets) - 1
        L, bad = None, np.zeros(G)
        for lo, hi, F, yt, V in self._score_chunks(W, x, y, member, max_bytes):
            if L is None:
                L = torch.empty((G, N * o), dtype=torch.float64, device=F.device)
            Lc, share = scoring.group_lpd(F, yt, sigma, offsets, V, loo=loo)
            L[:, lo * o:hi * o] = Lc
            if loo:
                bad += share * (hi - lo) / N
        res = scoring.stack_weights(L, tol=tol, max_iter=max_iter)
        self.stacking = {"weights": res["w"], "member_weights": stacking.member_weights(res["w"], offsets),
                         "elpd_stack": res["obj"], "elpd_equal": res["obj_equal"], "gap": res["gap"], "iters": res["iters"],
                         "n_dropped": res["n_dropped"], "n_nonfinite": res["n_nonfinite"],
                         "khat_bad_share": bad if loo else None, "offsets": np.asarray(offsets, dtype=np.int64)}
        return self.stacking

    def predict_mom_stacked(self, x, stacking=None, max_bytes=256 << 20):
        """(mean `(N, o)`, variance `(N, o)`) of the stacked predictive sum_m wm_m delta(f_m(x)) -- the weighted mean and the
        weighted variance sum wm (f - mean)^2 / (1 - sum wm^2) of the member predictions, without the data noise -- from
        MOMENTS-only calls of `qn_pred_score_w` on the members `stack` weighted (`stacking`: its dict; default the last one)."""
        stacking = self.stacking if stacking is None else stacking
        x = np.asarray(x, dtype=np.float64).reshape(len(x), -1)
        W = self._ens_weights_ordered(stacking["nsam"], **stacking["ens_args"])
        wm = None
        mean, var = [], []
        for lo, hi, F, _, _ in self._score_chunks(W, x, None, None, max_bytes):
            if wm is None:
                wm = torch.as_tensor(np.asarray(stacking["member_weights"], dtype=np.float64), device=F.device)
            rows = scoring.score_rows_w(F, None, 0.0, wm, None, _lib.SCORE_MOMENTS).cpu().numpy()
            mean.append(rows[4].reshape(hi - lo, -1))
            var.append(rows[5].reshape(hi - lo, -1))
        return np.concatenate(mean), np.concatenate(var)

    def score(self, x, y, noise=None, nsam=1000, crps=True, max_bytes=256 << 20, levels=scoring.DEFAULT_LEVELS, loo=False,
              member_weights=None, **ens_args):
        """Score the solver's `nsam`-member predictive ensemble against the targets y `(N, o)` at x: the dict of
        `scoring.summarise` (per entry lppd_k, p_waic_k, pit, crps_k, mean, var; scalars lppd, p_waic, elpd_waic, waic,
        se_elpd, nlpd, crps, rmse, coverage, pit_hist).  Member m predicts N(f_m(x), noise^2); `noise` defaults to the data
        noise of the last fit.  On the training data `waic` is the WAIC, on held-out data `nlpd` is the test negative log
        predictive density.  The weights are drawn ONCE (`_ens_weights`; ens_args as in `predict_ens`, e.g. NN_MCMC's
        `nburn`, `chain='all'`; a solver that sampled the noise level scores member m at its own level, through the
        per-member variance V of `qn_pred_score`, unless `noise` is given), then x is walked in row chunks whose `M x rows x o` predictions fit `max_bytes`: one batched
        forward and one `qn_pred_score` per chunk, and only `6 x rows x o` doubles are downloaded.  An entry's scores do
        not depend on the chunking.  crps=False skips the pair pass, which costs O(M^2) per entry.  loo=True adds the
        PSIS-LOO scores (`scoring.summarise_loo`: elpd_loo_k, khat, ess_k, pit_loo, elpd_loo, looic, se_elpd_loo, khat_threshold,
        n_khat_bad, khat_bad, coverage_loo, pit_loo_hist; and p_loo): one `qn_psis_loo` per chunk on the same F and V and
        `4 x rows x o` more doubles downloaded.  member_weights `(M,)` (>= 0, sum 1: `stack(...)['member_weights']`, with the
        nsam and ens_args `stack` was called with) scores the weighted mixture through `qn_pred_score_w` instead of the
        equal-weight one; the members then come in the reproducible order of `_ens_weights_ordered`.  Not together with loo."""
        if member_weights is not None and loo:
            raise ValueError("loo=True scores the equal-weight ensemble: not together with member_weights")
        member = self._score_member_noise(noise, nsam, **ens_args)
        sigma = self._score_noise(noise) if member is None else 0.0
        x = np.asarray(x, dtype=np.float64).reshape(len(x), -1)
        y = np.asarray(y, dtype=np.float64).reshape(len(x), -1)
        W = self._ens_weights(nsam, **ens_args) if member_weights is None else self._ens_weights_ordered(nsam, **ens_args)
        M, (N, o) = len(W), y.shape
        what = scoring.WHAT_ALL if crps else scoring.WHAT_ALL & ~_lib.SCORE_CRPS
        rows = np.empty((_lib.SCORE_NOUT, N * o))
        loo_rows = np.empty((_lib.LOO_NOUT, N * o)) if loo else None
        wm = None
        if member_weights is not None:
            wm = np.asarray(member_weights, dtype=np.float64).reshape(-1)
            if wm.shape != (M,):
                raise ValueError(f"member_weights holds {wm.size} weights for an ensemble of {M} members")
        for lo, hi, F, yt, V in self._score_chunks(W, x, y, member, max_bytes):
            if wm is not None:
                wm = torch.as_tensor(wm, device=F.device)
                rows[:, lo * o:hi * o] = scoring.score_rows_w(F, yt, sigma, wm, V, what).cpu().numpy()
                continue
            rows[:, lo * o:hi * o] = scoring.score_rows(F, yt, sigma, V, what).cpu().numpy()
            if loo:
                loo_rows[:, lo * o:hi * o] = scoring.psis_rows(F, yt, sigma, V).cpu().numpy()
        return scoring.summarise_all(rows, loo_rows, y, M, levels)

    # -- quantiles and credible bands of the predictive (qn_pred_quantile) ------------------------------------
    def predict_quantiles(self, x, q=(0.05, 0.5, 0.95), noise=None, nsam=1000, member_weights=None, max_bytes=256 << 20,
                          **ens_args):
        """`(Q, N, o)`: the quantiles at the levels q of the predictive that `score` judges -- member m of the solver's
        `nsam`-member ensemble predicts N(f_m(x), noise^2), mixed with equal weights or with member_weights `(M,)`
        (`stack(...)['member_weights']`, with the nsam and ens_args `stack` was called with; the members then come in the
        order of `_ens_weights_ordered`).  `noise` defaults to the data noise of the last fit (a solver that sampled the noise
        level: every member at its own level); noise=0 or False gives the epistemic order-statistic quantiles of the members,
        np.quantile's default method, where the levels may be 0 and 1.  The weights are drawn ONCE, then x is walked in the
        row chunks of `score`: one batched forward and one `qn_pred_quantile` per chunk, and only `Q x rows x o` doubles are
        downloaded.  An entry's quantiles do not depend on the chunking."""
        epistemic = noise is not None and float(noise) == 0.0
        member = None if epistemic else self._score_member_noise(noise, nsam, **ens_args)
        sigma = 0.0 if (epistemic or member is not None) else self._score_noise(noise)
        x = np.asarray(x, dtype=np.float64).reshape(len(x), -1)
        q = np.asarray(q, dtype=np.float64).reshape(-1)
        W = self._ens_weights(nsam, **ens_args) if member_weights is None else self._ens_weights_ordered(nsam, **ens_args)
        M, N = len(W), len(x)
        wm = None
        if member_weights is not None:
            wm = np.asarray(member_weights, dtype=np.float64).reshape(-1)
            if wm.shape != (M,):
                raise ValueError(f"member_weights holds {wm.size} weights for an ensemble of {M} members")
        out = None
        for lo, hi, F, _, V in self._score_chunks(W, x, None, member, max_bytes):
            if wm is not None:
                wm = torch.as_tensor(wm, device=F.device)
            rows = scoring.quantile_rows(F, q, sigma, V, wm).cpu().numpy().reshape(q.size, hi - lo, -1)
            if out is None:
                out = np.empty((q.size, N, rows.shape[2]))
            out[:, lo:hi] = rows
        return out

    def predict_interval(self, x, level=0.9, **kwargs):
        """(lo, median, hi), each `(N, o)`: the central credible band of the predictive at `level` and its median -- the
        quantiles (1 - level) / 2, 0.5 and (1 + level) / 2 of `predict_quantiles` (kwargs as there)."""
        level = float(level)
        if not 0.0 < level < 1.0:
            raise ValueError(f"level = {level}; 0 < level < 1 is needed")
        lo, mid, hi = self.predict_quantiles(x, q=(0.5 * (1.0 - level), 0.5, 0.5 * (1.0 + level)), **kwargs)
        return lo, mid, hi

    # -- figures (presentation only; same signatures and file names as quinn.py:106-260) ---------------
    @staticmethod
    def _center_and_spread(yens, quantiles):
        """(centre, lower, upper) of an ensemble: mean and +-std, or median and the distances to the quartiles."""
        if quantiles:
            q25, q50, q75 = np.quantile(yens, [0.25, 0.5, 0.75], axis=0)
            return q50, q50 - q25, q75 - q50
        sd = np.std(yens, axis=0)
        return np.mean(yens, axis=0), sd, sd

    def predict_plot(self, xx_list, yy_list, nmc=100, plot_qt=False, labels=None, colors=None, iouts=None, msize=14,
                     figname=None):
        """Predicted-vs-data ('diagonal') figure per output, error bars from an `nmc`-member ensemble;
        saved as `fitdiag_o<iout>.png` unless `figname` is given."""
        import matplotlib
        matplotlib.use("Agg", force=False)
        import matplotlib.pyplot as plt
        assert len(xx_list) == len(yy_list)
        stats = [self._center_and_spread(self.predict_ens(xx, nens=nmc), plot_qt) for xx in xx_list]
        nset, nout = len(xx_list), stats[0][0].shape[1]
        labels = labels or [f'Set {i + 1}' for i in range(nset)]
        colors = colors or (['b', 'g', 'r', 'c', 'm', 'y'] * nset)[:nset]
        for iout in (range(nout) if iouts is None else iouts):
            plt.figure(figsize=(10, 10))
            lo = min(float(yy[:, iout].min()) for yy in yy_list)
            hi = max(float(yy[:, iout].max()) for yy in yy_list)
            plt.plot([lo, hi], [lo, hi], 'k--', linewidth=1)
            for (mid, dl, du), yy, lab, col in zip(stats, yy_list, labels, colors):
                plt.errorbar(yy[:, iout], mid[:, iout], yerr=[dl[:, iout], du[:, iout]], fmt=col + 'o', markersize=msize / 2,
                             markeredgecolor='w', label=lab)
            plt.xlabel(f'Model output # {iout + 1}')
            plt.ylabel(f'Fit output # {iout + 1}')
            plt.legend()
            plt.savefig(figname or f'fitdiag_o{iout}.png')
            plt.close()

    def plot_1d_fits(self, xx_list, yy_list, domain=None, ngr=111, plot_qt=False, nmc=100, true_model=None,
                     labels=None, colors=None, name_postfix=''):
        """One-dimensional slices of the fit through the middle of the domain, one figure per (input, output),
        saved as `fit_d<idim>_o<iout>_<name_postfix>.png`: data, ensemble members, centre and spread band."""
        import matplotlib
        matplotlib.use("Agg", force=False)
        import matplotlib.pyplot as plt
        assert len(xx_list) == len(yy_list)
        nset = len(xx_list)
        labels = labels or [f'Set {i + 1}' for i in range(nset)]
        colors = colors or (['b', 'g', 'r', 'c', 'm', 'y'] * nset)[:nset]
        if domain is None:
            xall = np.vstack(xx_list)
            domain = np.stack([xall.min(axis=0), xall.max(axis=0)], axis=1)
        ndim, nout = xx_list[0].shape[1], yy_list[0].shape[1]
        mid_label, band_label = ('Median Pred.', 'Qtile') if plot_qt else ('Mean Pred.', 'St.Dev.')
        for idim in range(ndim):
            unit = np.full((ngr, ndim), 0.5)
            unit[:, idim] = np.linspace(0.0, 1.0, ngr)
            xgrid = unit * (domain[:, 1] - domain[:, 0]) + domain[:, 0]
            yens = self.predict_ens(xgrid, nens=nmc)
            mid, dl, du = self._center_and_spread(yens, plot_qt)
            for iout in range(nout):
                plt.figure(figsize=(12, 8))
                for xx, yy, lab, col in zip(xx_list, yy_list, labels, colors):
                    plt.plot(xx[:, idim], yy[:, iout], col + 'o', markersize=13, markeredgecolor='w', label=lab, zorder=1000)
                if true_model is not None:
                    plt.plot(xgrid[:, idim], true_model(xgrid, 0.0)[:, iout], 'k-', alpha=0.5, label='Truth')
                for member in yens:
                    plt.plot(xgrid[:, idim], member[:, iout], 'm--', linewidth=1, zorder=-10000)
                plt.plot(xgrid[:, idim], mid[:, iout], 'm-', linewidth=5, label=mid_label)
                plt.fill_between(xgrid[:, idim], mid[:, iout] - dl[:, iout], mid[:, iout] + du[:, iout], color='plum',
                                 alpha=0.9, zorder=-1000, label=band_label)
                plt.legend()
                plt.xlabel(f'Input # {idim + 1}')
                plt.ylabel(f'Output # {iout + 1}')
                plt.savefig(f'fit_d{idim}_o{iout}_{name_postfix}.png')
                plt.close()
