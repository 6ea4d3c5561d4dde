#!/usr/bin/env python
"""The reference's `examples/ex_ufit.py` call pattern on the MI355X path.

    python examples/ex_ufit.py {amcmc|hmc|stack|quantiles|pt|sghmc|prior|hyper|noise|ess|nuts|vi|ens|rms|laplace|laplace_ggn|laplace_kron|laplace_evidence|swag} [--quick] [--mlp]

Same data generation, same network (`RNet(3, 3, wp_function=Poly(0), ...)`, examples/ex_ufit.py:72-77
there; `--mlp` switches to the commented-out MLP alternative), same solver calls and keyword
arguments as the reference example (examples/ex_ufit.py:40-115); differences: many chains run at
once (`seeds=`), the MCMC branches pool their predictive ensemble over all chains (`chain='all'`)
and print how well the chains agree (split-R-hat / ESS of parameters, log-posterior and predictions),
`laplace_ggn` is the Laplace solver with the Gauss-Newton curvature (`la_type='ggn'`, positive definite by construction) and
prints its closed-form linearised predictive (`predict_glm`) beside the sampled one,
`laplace_kron` is the same with the Kronecker-factored Gauss-Newton (`la_type='kron'`: two small factors per layer, no p x p matrix),
`laplace_evidence` is a `la_type='kron'` fit at a deliberately wrong `datanoise` followed by `tune_hyper`: it prints the members'
log evidence before and after, the tuned scales and the held-out nlpd of `score_glm` before and after,
`sghmc` is the device-only stochastic-gradient HMC (`engine='device'`; every chain draws its own minibatch on the GPU, cyclical
step size, every 10th state stored; MLP network),
`stack` is the device HMC (`engine='device'`; MLP network) whose 8 chains are stacked (`NN_MCMC.stack`: PSIS-LOO density per chain,
EM for the weights on the device) and scored on the test rows with equal and with stacking weights,
`quantiles` is the same stacked device HMC, printing the 90 % credible band of the predictive on the test rows
(`predict_interval`: quantiles of the Gaussian mixture with the data noise, found on the device) -- its width, coverage and
interval score (`scoring.interval_summary`) with equal and with stacking weights, beside the epistemic band without the noise,
`pt` is the device HMC with replica exchange (`engine='device'`, 8 ladders of 4 rungs; predictions and diagnostics from the cold
chains; MLP network),
`prior` is the device HMC with the Gaussian weight prior `priorsigma=1.0` (`engine='device'`; MLP network), printed beside the same
run without a prior and a `laplace_ggn` fit with the same `priorsigma` -- the Laplace approximation of the posterior it samples,
`ess` is elliptical slice sampling on the device with the same `priorsigma=1.0` (`engine='device'`; MLP network): no step size, forward
calls only; it prints the forward evaluations a step took,
`nuts` is the No-U-Turn sampler on the device (`engine='device'`; MLP network): no trajectory length, the step size dual-averaged
over the first tenth of the run; it prints the depth and the leapfrogs a step took; `nuts mass` adds the mass windows of NUTS's own
warm-up (`adapt_mass=True`) and prints the range of the scales found,
and the matplotlib output is replaced by a printed summary of the predictive mean / standard deviation.
"""
import sys

import numpy as np
import torch

from quinn_amd.nns.mlp import MLP
from quinn_amd.nns.rnet import RNet, Poly
from quinn_amd.solvers.nn_ens import NN_Ens
from quinn_amd.solvers.nn_rms import NN_RMS
from quinn_amd.solvers.nn_laplace import NN_Laplace
from quinn_amd.solvers.nn_swag import NN_SWAG
from quinn_amd.solvers.nn_mcmc import NN_MCMC
from quinn_amd.solvers.nn_vi import NN_VI


def scale01ToDom(xx, dom):
    return xx * np.abs(dom[:, 1] - dom[:, 0]) + np.min(dom, axis=1)


def Sine(xx, datanoise=0.0):
    yy = datanoise * np.random.randn(xx.shape[0], 1)
    yy += np.sum(np.sin(xx), axis=1).reshape(-1, 1)
    return yy


def main(meth, quick=False, mlp=False, mass=False):
    torch.set_default_dtype(torch.double)
    all_uq_options = ['amcmc', 'hmc', 'stack', 'quantiles', 'pt', 'sghmc', 'prior', 'hyper', 'noise', 'ess', 'nuts', 'vi', 'ens', 'rms', 'laplace', 'laplace_ggn', 'laplace_kron', 'laplace_evidence', 'swag']
    assert meth in all_uq_options, f'Pick among {all_uq_options}'
    nall, trn_factor, ntst, ndim, datanoise = 15, 0.9, 13, 1, 0.02
    if meth == 'laplace_evidence':       # the evidence's fixed point needs more entries of y than effective parameters
        nall = 150
    domain = np.tile(np.array([-np.pi, np.pi]), (ndim, 1))
    xall = scale01ToDom(np.random.rand(nall, ndim), domain)
    yall = Sine(xall, datanoise=datanoise)
    np.random.seed(100)
    xtst = scale01ToDom(np.random.rand(ntst, ndim), domain)
    ytst = Sine(xtst, datanoise=datanoise)
    if mlp or meth in ('laplace', 'laplace_ggn', 'laplace_kron', 'laplace_evidence', 'sghmc', 'stack', 'quantiles', 'pt', 'prior', 'hyper', 'noise', 'ess', 'nuts'):    # the Laplace curvature kernels take MLPs (RNet is not covered); sghmc runs the MLP too
        nnet = MLP(ndim, 1, (11, 11, 11), biasorno=True, activ='tanh')
    else:
        nnet = RNet(3, 3, wp_function=Poly(0), indim=ndim, outdim=1, layer_pre=True, layer_post=True,
                    biasorno=True, nonlin=True, mlp=False, final_layer=None)
    ntrn = int(trn_factor * nall)
    xtrn, xval = xall[:ntrn, :], xall[ntrn:, :]
    ytrn, yval = yall[:ntrn, :], yall[ntrn:, :]
    k = 20 if quick else 1

    if meth == 'amcmc':
        uqnet = NN_MCMC(nnet, verbose=not quick)
        uqnet.fit(xtrn, ytrn, zflag=False, datanoise=datanoise, nmcmc=10000 // k, sampler='amcmc',
                  sampler_params={'gamma': 0.01}, seeds=range(8), diagnostics=True)
        predict = lambda x: uqnet.predict_ens(x, nens=100 // k * 2, nburn=1000 // k, chain='all')
    elif meth == 'hmc':
        uqnet = NN_MCMC(nnet, verbose=not quick)
        uqnet.fit(xtrn, ytrn, zflag=False, datanoise=datanoise, nmcmc=10000 // k, sampler='hmc',
                  sampler_params={'L': 3, 'epsilon': 0.0025}, seeds=range(8), diagnostics=True)
        predict = lambda x: uqnet.predict_ens(x, nens=100 // k * 2, nburn=1000 // k, chain='all')
    elif meth == 'stack':
        # 8 device HMC chains from different seeds; they do not mix, so they are stacked instead of pooled with equal weights
        uqnet = NN_MCMC(nnet, verbose=not quick)
        uqnet.fit(xtrn, ytrn, zflag=False, datanoise=datanoise, nmcmc=10000 // k, sampler='hmc', engine='device',
                  sampler_params={'L': 3, 'epsilon': 0.0025}, seeds=range(8), diagnostics=True)
        ens = dict(nsam=100 // k * 8, nburn=1000 // k)
        predict = lambda x: uqnet.predict_ens(x, nens=ens['nsam'], nburn=ens['nburn'], chain='all')
        st = uqnet.stack(xtrn, ytrn, loo=True, **ens)
        print("  stacking weights of the chains:", np.round(st['weights'], 4), f"({st['iters']} EM iterations, gap {st['gap']:.1e} nats)")
        print(f"  elpd_loo of the stacked mixture {st['elpd_stack']:.3f}, of the equal-weight pool {st['elpd_equal']:.3f}; "
              f"share of entries with an unreliable khat per chain: {np.round(st['khat_bad_share'], 2)}")
        for label, wm in (('equal weights', None), ('stacked', st['member_weights'])):
            sc = uqnet.score(xtst, ytst, chain='all', member_weights=wm, **ens)
            print(f"  test scores, {label}: nlpd {sc['nlpd']:.3f}  crps {sc['crps']:.4f}  rmse {sc['rmse']:.4f}  "
                  f"90 % coverage {sc['coverage'][0.9]:.2f}")
        sm, sv = uqnet.predict_mom_stacked(xtst)
        print(f"  stacked predictive on the test rows: mean |mean - y| {np.mean(np.abs(sm - ytst)):.4f}, mean std {np.mean(np.sqrt(sv)):.4f}")
    elif meth == 'quantiles':
        from quinn_amd import scoring
        uqnet = NN_MCMC(nnet, verbose=not quick)
        uqnet.fit(xtrn, ytrn, zflag=False, datanoise=datanoise, nmcmc=10000 // k, sampler='hmc', engine='device',
                  sampler_params={'L': 3, 'epsilon': 0.0025}, seeds=range(8), diagnostics=True)
        ens = dict(nsam=100 // k * 8, nburn=1000 // k)
        predict = lambda x: uqnet.predict_ens(x, nens=ens['nsam'], nburn=ens['nburn'], chain='all')
        st = uqnet.stack(xtrn, ytrn, loo=True, **ens)
        print("  stacking weights of the chains:", np.round(st['weights'], 4))
        for label, wm in (('equal weights', None), ('stacked', st['member_weights'])):
            lo, med, hi = uqnet.predict_interval(xtst, level=0.9, chain='all', member_weights=wm, **ens)
            band = scoring.interval_summary(lo, hi, ytst, 0.9)
            print(f"  90 % band on the test rows, {label}: width {band['width']:.4f}  coverage {band['coverage']:.2f}  "
                  f"interval score {band['interval_score']:.4f}  mean |median - y| {np.mean(np.abs(med - ytst)):.4f}")
        lo, _, hi = uqnet.predict_interval(xtst, level=0.9, noise=0, chain='all', **ens)
        print(f"  epistemic 90 % band (no data noise, order statistics of the members): width {np.mean(hi - lo):.4f}")
    elif meth == 'pt':
        uqnet = NN_MCMC(nnet, verbose=not quick)
        uqnet.fit(xtrn, ytrn, zflag=False, datanoise=datanoise, nmcmc=10000 // k, sampler='hmc', engine='device',
                  sampler_params={'L': 3, 'epsilon': 0.0025, 'ladder': 4, 'beta_min': 0.05}, seeds=range(32), diagnostics=True)
        predict = lambda x: uqnet.predict_ens(x, nens=100 // k * 2, nburn=1000 // k, chain='all')
        r = uqnet.mcmc_results
        print("  swap acceptance per rung pair:", np.round(r['swap_rate'].reshape(-1, 4)[:, :-1].mean(axis=0), 3))
    elif meth == 'sghmc':
        uqnet = NN_MCMC(nnet, verbose=not quick)
        uqnet.fit(xtrn, ytrn, zflag=False, datanoise=datanoise, nmcmc=10000 // k, sampler='sghmc', engine='device',
                  sampler_params={'eta': 4e-6, 'alpha': 0.1, 'batch': 8, 'thin': 10, 'schedule': 'cyclic', 'cycles': 4,
                                  'explore_frac': 0.25}, seeds=range(8), diagnostics=True)
        predict = lambda x: uqnet.predict_ens(x, nens=100 // k * 2, nburn=1000 // k, chain='all')
    elif meth == 'prior':
        others, ps = {}, 1.0
        xg = scale01ToDom(np.linspace(0.0, 1.0, 11), domain)[:, np.newaxis]
        for label, prior in (('no prior', None), ('priorsigma = %g' % ps, ps)):      # (the fit with the prior last: it is `uqnet`)
            uqnet = NN_MCMC(nnet, verbose=not quick)
            uqnet.fit(xtrn, ytrn, zflag=False, datanoise=datanoise, nmcmc=10000 // k, sampler='hmc', engine='device',
                      sampler_params={'L': 3, 'epsilon': 0.0025}, seeds=range(8), diagnostics=True, priorsigma=prior)
            ye = uqnet.predict_ens(xg, nens=100 // k * 2, nburn=1000 // k, chain='all')
            others['HMC, ' + label] = (ye.mean(axis=0)[:, 0], ye.std(axis=0, ddof=1)[:, 0])
            w = uqnet.samples[:, 1000 // k:].reshape(-1, uqnet.pdim)
            print(f"  HMC, {label}: mean |w|^2 / p over the kept rows {np.mean(w * w):.4f}, best log-posterior "
                  f"{np.max(uqnet.mcmc_results['maxpost']):.2f}")
        predict = lambda x: uqnet.predict_ens(x, nens=100 // k * 2, nburn=1000 // k, chain='all')
        la = NN_Laplace(nnet, nens=3, dfrac=1.0, verbose=not quick, la_type='ggn', datanoise=datanoise, priorsigma=ps)
        la.fit(xtrn, ytrn, val=[xval, yval], lrate=0.01, batch_size=2, nepochs=1000 // k, freq_out=1000)
        yl = la.predict_ens(xg, nens=111)
        others['laplace_ggn, priorsigma = %g' % ps] = (yl.mean(axis=0)[:, 0], yl.std(axis=0, ddof=1)[:, 0])
        for label, (m, s) in others.items():
            print(f"  {label}: predictive std on the grid " + " ".join(f"{v:.3f}" for v in s))
    elif meth == 'hyper':
        # a precision per layer with a Gamma(1, 1) hyper-prior, Gibbs-sampled on the device after every HMC step
        uqnet = NN_MCMC(nnet, verbose=not quick)
        uqnet.fit(xtrn, ytrn, zflag=False, datanoise=datanoise, nmcmc=10000 // k, sampler='hmc', engine='device',
                  sampler_params={'L': 3, 'epsilon': 0.0025}, seeds=range(8), diagnostics=True,
                  hyperprior=dict(a0=1.0, b0=1.0, groups='layer'))
        predict = lambda x: uqnet.predict_ens(x, nens=100 // k * 2, nburn=1000 // k, chain='all')
        r = uqnet.mcmc_results
        for (name, lo, hi), t in zip(r['prior_groups'], r['tau'][:, (1000 // k):].mean(axis=(0, 1))):
            print(f"  {name} (weights {lo} .. {hi - 1}): posterior mean precision {t:.3f} (prior scale {t ** -0.5:.3f})")
    elif meth == 'noise':
        # no hand-set scale.  Gibbs-sampling the noise from a random start finds the 'everything is noise' mode (a large SSE draws
        # a large noise level, at which the weights barely move), so a first run at a fixed, ten times too large noise level
        # brings the chains to the data; the second starts where it ended and samples the noise level after every HMC step
        # (the weight scale per layer likewise, in both runs)
        uqnet = NN_MCMC(nnet, verbose=not quick)
        common = dict(zflag=False, datanoise=10 * datanoise, nmcmc=10000 // k, sampler='hmc', engine='device',
                      sampler_params={'L': 3, 'epsilon': 0.0025}, seeds=range(8), hyperprior=dict(a0=1.0, b0=1.0, groups='layer'))
        uqnet.fit(xtrn, ytrn, **common)
        uqnet.fit(xtrn, ytrn, param_ini=uqnet.samples[:, -1], diagnostics=True, noiseprior=dict(a0=2.0, b0=1e-3), **common)
        predict = lambda x: uqnet.predict_ens(x, nens=100 // k * 2, nburn=1000 // k, chain='all')
        sig = uqnet.mcmc_results['sigma'][:, (1000 // k):]
        print(f"  noise level: started at {10 * datanoise:g}, posterior mean {sig.mean():.4f} "
              f"(5 % .. 95 %: {np.quantile(sig, 0.05):.4f} .. {np.quantile(sig, 0.95):.4f}); the data's is {datanoise:g}")
        sc = uqnet.score(xtst, ytst, nsam=100 // k * 2, nburn=1000 // k, chain='all')
        print(f"  test nlpd at the sampled levels {sc['nlpd']:.3f}, 90 % coverage {sc['coverage'][0.9]:.2f}")
    elif meth == 'nuts':
        uqnet = NN_MCMC(nnet, verbose=not quick)
        uqnet.fit(xtrn, ytrn, zflag=False, datanoise=datanoise, nmcmc=10000 // k, sampler='nuts', engine='device',
                  sampler_params={'epsilon': 1e-3, 'adapt': 1000 // k, 'max_depth': 8, **({'adapt_mass': True} if mass else {})},
                  seeds=range(8), diagnostics=True)
        predict = lambda x: uqnet.predict_ens(x, nens=100 // k * 2, nburn=1000 // k, chain='all')
        r = uqnet.mcmc_results
        print(f"  depth per step: mean {r['depth'][:, 1:].mean():.2f}, max {r['depth'].max()}; leapfrogs per step: mean "
              f"{r['nleap'][:, 1:].mean():.2f}; divergent steps {r['ndiv'].sum()}, stopped by max_depth {r['ntreedepth'].sum()}; "
              f"step sizes {r['epsilon'].min():.3g} .. {r['epsilon'].max():.3g}; acceptance statistic {r['accrate'].mean():.3f}")
        if r.get('mass_scale') is not None:
            print(f"  mass windows: scales {r['mass_scale'].min():.3g} .. {r['mass_scale'].max():.3g}")
    elif meth == 'ess':
        uqnet = NN_MCMC(nnet, verbose=not quick)
        uqnet.fit(xtrn, ytrn, zflag=False, datanoise=datanoise, nmcmc=10000 // k, sampler='ess', engine='device',
                  sampler_params={'max_shrink': 32}, seeds=range(8), diagnostics=True, priorsigma=1.0)
        predict = lambda x: uqnet.predict_ens(x, nens=100 // k * 2, nburn=1000 // k, chain='all')
        r = uqnet.mcmc_results
        print(f"  forward evaluations per step: mean {r['nev'][:, 1:].mean():.2f}, max {r['nev'].max()}; truncated steps "
              f"{int(r['ntrunc'].sum())}; best log-posterior {np.max(r['maxpost']):.2f}")
    elif meth == 'vi':
        uqnet = NN_VI(nnet, verbose=not quick)
        uqnet.fit(xtrn, ytrn, val=[xval, yval], datanoise=datanoise, lrate=0.01, batch_size=None, nsam=1,
                  nepochs=5000 // k, freq_out=1000)
        predict = lambda x: uqnet.predict_ens(x, nens=111)
    elif meth == 'ens':
        uqnet = NN_Ens(nnet, nens=3, dfrac=0.8, verbose=not quick)
        uqnet.fit(xtrn, ytrn, val=[xval, yval], lrate=0.01, batch_size=2, nepochs=1000 // k, freq_out=1000)
        predict = lambda x: uqnet.predict_ens(x)
    elif meth == 'laplace':
        uqnet = NN_Laplace(nnet, nens=3, dfrac=1.0, verbose=not quick, la_type='full')
        uqnet.fit(xtrn, ytrn, val=[xval, yval], lrate=0.01, batch_size=2, nepochs=1000 // k, freq_out=1000)
        predict = lambda x: uqnet.predict_ens(x, nens=111)
    elif meth == 'laplace_ggn':
        uqnet = NN_Laplace(nnet, nens=3, dfrac=1.0, verbose=not quick, la_type='ggn', datanoise=datanoise)
        uqnet.fit(xtrn, ytrn, val=[xval, yval], lrate=0.01, batch_size=2, nepochs=1000 // k, freq_out=1000)
        predict = lambda x: uqnet.predict_ens(x, nens=111)
    elif meth == 'laplace_kron':
        uqnet = NN_Laplace(nnet, nens=3, dfrac=1.0, verbose=not quick, la_type='kron', datanoise=datanoise)
        uqnet.fit(xtrn, ytrn, val=[xval, yval], lrate=0.01, batch_size=2, nepochs=1000 // k, freq_out=1000)
        predict = lambda x: uqnet.predict_ens(x, nens=111)
    elif meth == 'laplace_evidence':
        # a 'kron' fit at a deliberately wrong noise level (10 x the data's), then the noise level and the per-layer prior
        # precisions that maximise every member's Laplace evidence at its MAP weights; the MAP weights are not refitted
        uqnet = NN_Laplace(nnet, nens=3, dfrac=1.0, verbose=not quick, la_type='kron', datanoise=10 * datanoise)
        uqnet.fit(xtrn, ytrn, val=[xval, yval], lrate=0.01, batch_size=15, nepochs=1000 // k, freq_out=1000)
        nlpd_before = uqnet.score_glm(xtst, ytst)['nlpd']
        tuned = uqnet.tune_hyper(groups='layer')
        print("  log evidence of the members at the fit's scales:", np.round(tuned['logZ_start'], 3))
        print("  ... and at their tuned scales:                  ", np.round(tuned['logZ'], 3),
              f"(iterations {tuned['iters']}, converged {tuned['converged']})")
        print(f"  datanoise of the fit {uqnet.datanoise:g}, tuned per member:", np.round(tuned['datanoise'], 4))
        print("  prior precisions per layer, tuned per member (the fit's: %g):" % (1.0 / uqnet.priorsigma ** 2))
        for row in tuned['prior_prec']:
            print("   ", np.round(row, 4))
        print("  effective number of parameters per member:", np.round(tuned['gamma'].sum(axis=1), 2), f"of {uqnet.nparams}")
        print(f"  nlpd of the linearised predictive on the held-out rows: {nlpd_before:.4f} before, "
              f"{uqnet.score_glm(xtst, ytst)['nlpd']:.4f} after")
        print("  evidence weights of the members:", np.round(uqnet.evidence_weights(), 4))
        predict = lambda x: uqnet.predict_ens(x, nens=111)
    elif meth == 'swag':
        uqnet = NN_SWAG(nnet, nens=3, dfrac=1.0, verbose=not quick, k=10, n_steps=12, c=1, cov_type="lowrank",
                        lr_swag=0.01)
        uqnet.fit(xtrn, ytrn, val=[xval, yval], lrate=0.01, batch_size=2, nepochs=1000 // k, freq_out=1000)
        predict = lambda x: uqnet.predict_ens(x, nens=111)
    else:
        uqnet = NN_RMS(nnet, nens=7, dfrac=1.0, verbose=not quick, datanoise=datanoise, priorsigma=0.1)
        uqnet.fit(xtrn, ytrn, val=[xval, yval], lrate=0.01, batch_size=2, nepochs=1000 // k, freq_out=1000)
        predict = lambda x: uqnet.predict_ens(x)

    xgrid = scale01ToDom(np.linspace(0.0, 1.0, 11), domain)[:, np.newaxis]
    y = predict(xgrid)
    ymean, ystd = y.mean(axis=0)[:, 0], y.std(axis=0, ddof=1)[:, 0]
    print(f"{meth}: {y.shape[0]} predictive samples on an 11-point grid")
    for xg, m, s, t in zip(xgrid[:, 0], ymean, ystd, np.sin(xgrid[:, 0])):
        print(f"  x={xg:+.3f}  mean={m:+.4f}  std={s:.4f}  truth={t:+.4f}")
    if meth in ('laplace_ggn', 'laplace_kron', 'laplace_evidence'):
        gmean, gvar, _ = uqnet.predict_glm(xgrid, msc=1)
        print("  linearised (GLM) predictive in closed form beside the sampled one:")
        for xg, m, s, gm, gs in zip(xgrid[:, 0], ymean, ystd, gmean[:, 0], np.sqrt(gvar[:, 0])):
            print(f"  x={xg:+.3f}  sampled mean={m:+.4f} std={s:.4f}   glm mean={gm:+.4f} std={gs:.4f}")
    rmse = float(np.sqrt(np.mean((uqnet.predict_ens(xtst, nens=y.shape[0]).mean(axis=0) - ytst) ** 2))) \
        if meth in ('vi', 'ens', 'rms', 'laplace', 'laplace_ggn', 'laplace_kron', 'laplace_evidence', 'swag') else float(np.sqrt(np.mean((predict(xtst).mean(axis=0) - ytst) ** 2)))
    print(f"  test RMSE of the predictive mean: {rmse:.4f}")
    if meth in ('amcmc', 'hmc', 'stack', 'pt', 'sghmc', 'prior', 'hyper', 'noise', 'ess', 'nuts'):
        dg = dict(uqnet.diagnostics, pred=uqnet.diagnose(xgrid, nburn=1000 // k, nens=100 // k * 2)['pred'])
        for name, label in (('params', 'parameters'), ('logpost', 'log-posterior'), ('pred', 'predictions on the grid')):
            d = dg[name]
            print(f"  {label}: max R-hat {np.nanmax(d['rhat']):.3f}  min ESS {np.nanmin(d['ess']):.1f} of {d['n_draws']} draws"
                  f" ({d['rhat'].size} entries, 8 chains)")     # (pt: the 8 cold chains of 32)
    return ymean, ystd, rmse


if __name__ == '__main__':
    torch.manual_seed(0)
    np.random.seed(0)
    main(sys.argv[1], quick='--quick' in sys.argv, mlp='--mlp' in sys.argv, mass='mass' in sys.argv[2:])
