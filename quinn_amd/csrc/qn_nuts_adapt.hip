// The windowed warm-up of the device No-U-Turn sampler: per-chain step size (dual averaging) and per-chain diagonal mass
// (Welford moments over Stan's slow windows) for chains that each run on their own step counter.
//   qn_nuts_adapt : one launch behind each qn_nuts_iter (called with adapt = 0) while a chain can still be in warm-up
// include/quinn_amd_nuts_adapt.h has the contract, quinn_amd/mcmc/nuts_adapt.py restates it in numpy.  qn_nuts.hip is left as
// it is: this kernel reads both slots of the chains' counters to see which chain ended a step, looks the chain's own warm-up
// step up in a plan table, and amends what the iteration wrote -- the step size of the fresh slot, the scale, and the first
// half kick and drift of the step that has just started.
// Geometry of the NUTS kernels: hmc_parts(p) workgroups of HBLK threads per chain, the same pair of elements per thread, so
// mean / m2 / scale / q / u are updated in place by their owner.  The scalars are read from ws[parity] by every workgroup and
// written, by workgroup 0 alone, to ws[1 - parity]; es.eps is written by workgroup 0 and read by nobody here: no workgroup
// sees a half-updated chain, no atomics, no fences, plain vector stores.  FP contraction is off for the whole file: every
// elementwise operation takes one rounding, as in numpy.
#include "qn_mcmc_shared.h"
#include "../../include/quinn_amd_nuts_adapt.h"

#pragma clang fp contract(off)

namespace {

constexpr int NES = 12, NEI = 8, NWS = 4;      // es, ei as in qn_nuts.hip (eps is es[0]; t is ei[0], v ei[3]); ws: mu, hbar, logbar, eps

struct WarmArgs {
    double gs, target;                         // -0.5 / sigma^2, target_accept
    int C, nmcmc, adapt, par;
    int64_t p;
};

struct WarmVec {                               // [C, p]
    const double *cur, *ql, *ul, *gl;
    double *q, *u, *mean, *m2, *scale;
};

__global__ __launch_bounds__(HBLK) void k_nuts_adapt(WarmArgs a, WarmVec w, const double* __restrict__ alphas,
                                                     const int32_t* __restrict__ plan, double* __restrict__ es,
                                                     const int64_t* __restrict__ ei, double* ws) {
    const int b = blockIdx.y;
    const int64_t so = (int64_t)a.par * a.C + b, sn = (int64_t)(1 - a.par) * a.C + b;
    const bool w0 = blockIdx.x == 0 && threadIdx.x == 0;
    const double* win = ws + so * NWS;
    double* wout = ws + sn * NWS;
    double mu = win[0], hbar = win[1], logbar = win[2];
    const int64_t k = ei[sn * NEI];            // completed steps after the iteration
    bool live = k == ei[so * NEI] + 1 && k >= 1 && k <= a.adapt;                // (adapt <= nmcmc: k indexes plan and alphas)
    int m = 0, n = 0, flags = 0;
    if (live) {
        m = plan[4 * (k - 1)]; n = plan[4 * (k - 1) + 1]; flags = plan[4 * (k - 1) + 2];
        live = m >= 1 && !((flags & QN_NUTS_PLAN_COLLECT) && n < 1) && !((flags & QN_NUTS_PLAN_FINISH) && n < 2);
    }
    if (!live) {                               // not touched: the scalars are carried over
        if (w0) { wout[0] = mu; wout[1] = hbar; wout[2] = logbar; wout[3] = win[3]; }
        return;
    }
    const bool collect = flags & QN_NUTS_PLAN_COLLECT, finish = flags & QN_NUTS_PLAN_FINISH, freeze = flags & QN_NUTS_PLAN_FREEZE;
    // ---- the scalars: every workgroup of the chain forms the same numbers (HostAdaptation.update, operation by operation)
    const double mh = alphas[(int64_t)b * (a.nmcmc + 1) + k];
    const double acc = mh == mh ? fmin(1.0, mh) : 0.0, md = (double)m;
    hbar = (1.0 - 1.0 / (md + 10.0)) * hbar + (a.target - acc) / (md + 10.0);
    const double logeps = mu - (sqrt(md) / 0.05) * hbar, eta = pow(md, -0.75);
    logbar = eta * logeps + (1.0 - eta) * logbar;
    const double eps = exp(freeze ? logbar : logeps);
    if (w0) {
        if (finish) { mu = log(10.0 * eps); hbar = 0.0; logbar = 0.0; }
        wout[0] = mu; wout[1] = hbar; wout[2] = logbar; wout[3] = eps;
        es[sn * NES] = eps;
    }
    const bool next = k < a.nmcmc;             // the next step has started: its first half kick and drift again
    if (!collect && !finish && !next) return;
    const double v = (double)ei[sn * NEI + 3];
    const double hk = v * ((0.5 * eps) * a.gs), dr = v * eps;
    const double nd = (double)n, nm1 = nd - 1.0, c0 = nd / (nd + 5.0), c1 = (1e-3 * 5.0) / (nd + 5.0);
    const int64_t base = (int64_t)b * a.p, npair = (a.p + 1) / 2;
    const int64_t pchunk = (npair + gridDim.x - 1) / gridDim.x, lo = blockIdx.x * pchunk;
    const int64_t hi = lo + pchunk < npair ? lo + pchunk : npair;
    for (int64_t j = lo + threadIdx.x; j < hi; j += HBLK) {
        const int64_t e = 2 * j, o = base + e;
        const bool both = e + 1 < a.p;
        d2u s = ld2(w.scale + o, both);
        if (collect || finish) {
            d2u mn = ld2(w.mean + o, both), s2 = ld2(w.m2 + o, both);
            if (collect) {
                const d2u x = ld2(w.cur + o, both);
                const double d0 = x.x - mn.x, d1 = x.y - mn.y;
                mn.x = mn.x + d0 / nd; mn.y = mn.y + d1 / nd;
                s2.x = s2.x + d0 * (x.x - mn.x); s2.y = s2.y + d1 * (x.y - mn.y);
            }
            if (finish) {
                s.x = sqrt((c0 * s2.x) / nm1 + c1); s.y = sqrt((c0 * s2.y) / nm1 + c1);
                st2(w.scale + o, s.x, s.y, both);
                mn.x = mn.y = s2.x = s2.y = 0.0;
            }
            st2(w.mean + o, mn.x, mn.y, both);
            st2(w.m2 + o, s2.x, s2.y, both);
        }
        if (next) {
            const d2u qe = ld2(w.ql + o, both), ue = ld2(w.ul + o, both), ge = ld2(w.gl + o, both);
            const double u0 = ue.x + (hk * s.x) * ge.x, u1 = ue.y + (hk * s.y) * ge.y;
            st2(w.u + o, u0, u1, both);
            st2(w.q + o, qe.x + (dr * s.x) * u0, qe.y + (dr * s.y) * u1, both);
        }
    }
}

}  // namespace

extern "C" int qn_nuts_adapt(const double* cur, const double* alphas, int nmcmc, int adapt, double target_accept,
                             const int32_t* plan, double* es, const int64_t* ei, int parity, int C, int64_t p, double sigma,
                             const double* ql, const double* ul, const double* gl, double* q, double* u, double* ws,
                             double* mean, double* m2, double* scale, void* stream) {
    if (C < 1 || C > 65535 || p < 1 || nmcmc < 1) {
        qn_set_error("qn_nuts_adapt: bad size (1 <= C = %d <= 65535, p = %lld >= 1, nmcmc = %d >= 1)", C, (long long)p, nmcmc);
        return QN_EINVAL;
    }
    if (!(sigma > 0.0) || !std::isfinite(sigma)) {
        qn_set_error("qn_nuts_adapt: sigma = %g must be > 0 and finite", sigma);
        return QN_EINVAL;
    }
    if (adapt < 1 || adapt > nmcmc || (parity != 0 && parity != 1) || !(target_accept > 0.0 && target_accept < 1.0)) {
        qn_set_error("qn_nuts_adapt: adapt = %d in 1 .. nmcmc = %d, target_accept = %g in (0, 1), parity = %d 0 or 1", adapt,
                     nmcmc, target_accept, parity);
        return QN_EINVAL;
    }
    if (!cur || !alphas || !plan || !es || !ei || !ql || !ul || !gl || !q || !u || !ws || !mean || !m2 || !scale) {
        qn_set_error("qn_nuts_adapt: a NULL pointer (only stream may be NULL)");
        return QN_EINVAL;
    }
    WarmArgs a;
    a.gs = -0.5 / (sigma * sigma); a.target = target_accept;
    a.C = C; a.nmcmc = nmcmc; a.adapt = adapt; a.par = parity; a.p = p;
    const WarmVec w = {cur, ql, ul, gl, q, u, mean, m2, scale};
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_nuts_adapt, dim3(hmc_parts(p), C), dim3(HBLK), 0, static_cast<hipStream_t>(stream), a, w, alphas, plan,
                       es, ei, ws);
    QN_HIP_CHECK(hipGetLastError());
    return QN_OK;
}
