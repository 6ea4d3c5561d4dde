// The warm-up of device HMC / MALA with a per-chain step size and a diagonal mass matrix:
//   qn_hmc_adapt : one launch per warm-up step after the accept call: dual averaging of the step size (Hoffman & Gelman 2014,
//                  algorithm 5) and Welford moments of the state for the scale
// It writes the arrays eps [C] and scale [C, p] that qn_hmc_begin_s / qn_hmc_leap_s read (qn_hmc_leap.hip, which states the
// whitened leapfrog they run).  All stores are ordinary vector stores, no atomics, no fences.
#include "qn_mcmc_shared.h"

namespace {

// One warm-up step's adaptation.  Scalars (workgroup 0 of the chain, thread 0): the acceptance of the step just decided
// is alphas[c, t] with t = step_ptr[par] (the slot the accept call wrote); a = min(1, mh), NaN -> 0;
//   Hbar = (1 - w) Hbar + (target - a) w;  logeps = mu - sg Hbar;  logbar = eta logeps + (1 - eta) logbar
// with the host-computed w = 1 / (m + t0), sg = sqrt(m) / gamma, eta = m^-kappa; eps_c = exp(logeps), or exp(logbar) when
// the warm-up ends (freeze); at a window end (finish) dual averaging restarts around the new step: mu = log(10 eps_c),
// Hbar = logbar = 0.  da [C, 4] = (mu, Hbar, logbar, logeps).
// Elements (all workgroups of the chain, pairs of elements as 16-byte accesses): collect -- Welford update with the
// host-known count n; finish -- scale = sqrt(c0 * M2 / (n - 1) + c1), then mean = M2 = 0.
struct AdaptArgs {
    int nmcmc, par, collect, finish, freeze;
    int64_t p;
    double w, sg, eta, target;
    double n, nm1, c0, c1;          // n, n - 1, n / (n + 5), 1e-3 * 5 / (n + 5)
};
constexpr int WPT = 2;              // pairs per thread and pass
__global__ __launch_bounds__(HBLK) void k_hmc_adapt(AdaptArgs a, const double* __restrict__ cur,
                                                    const double* __restrict__ alphas,
                                                    const int64_t* __restrict__ step_ptr, double* __restrict__ da,
                                                    double* __restrict__ eps, double* __restrict__ mean,
                                                    double* __restrict__ m2, double* __restrict__ scale) {
    const int b = blockIdx.y;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const int64_t t = step_ptr[a.par];
        const double mh = (t >= 0 && t <= a.nmcmc) ? alphas[(int64_t)b * (a.nmcmc + 1) + t] : 0.0;
        const double acc = (mh == mh) ? fmin(1.0, mh) : 0.0;                 // NaN (a diverged trajectory) counts as 0
        double mu = da[4 * b], hbar = da[4 * b + 1], logbar = da[4 * b + 2];
        hbar = (1.0 - a.w) * hbar + (a.target - acc) * a.w;
        const double logeps = mu - a.sg * hbar;
        logbar = a.eta * logeps + (1.0 - a.eta) * logbar;
        const double e = a.freeze ? exp(logbar) : exp(logeps);
        if (a.finish) { mu = log(10.0 * e); hbar = 0.0; logbar = 0.0; }
        da[4 * b] = mu; da[4 * b + 1] = hbar; da[4 * b + 2] = logbar; da[4 * b + 3] = logeps;
        eps[b] = e;
    }
    if (!a.collect && !a.finish) return;
    const int64_t base = (int64_t)b * a.p;
    const int64_t npair = (a.p + 1) / 2;
    const int64_t stride = (int64_t)gridDim.x * (WPT * HBLK);
    for (int64_t pair0 = (int64_t)blockIdx.x * (WPT * HBLK) + threadIdx.x; pair0 < npair; pair0 += stride) {
        d2u xv[WPT], mv[WPT], sv[WPT];
#pragma unroll
        for (int h = 0; h < WPT; ++h) {
            const int64_t pair = pair0 + (int64_t)h * HBLK, e = 2 * pair;
            const bool in = pair < npair, both = e + 1 < a.p;
            const d2u zero = {0.0, 0.0};
            xv[h] = (in && a.collect) ? ld2(cur + base + e, both) : zero;
            mv[h] = (in && a.collect) ? ld2(mean + base + e, both) : zero;
            sv[h] = in ? ld2(m2 + base + e, both) : zero;
        }
#pragma unroll
        for (int h = 0; h < WPT; ++h) {
            const int64_t pair = pair0 + (int64_t)h * HBLK, e = 2 * pair;
            if (pair >= npair) break;
            const bool both = e + 1 < a.p;
            d2u mn = mv[h], s2 = sv[h];
            if (a.collect) {
                const double d0 = xv[h].x - mn.x, d1 = xv[h].y - mn.y;
                mn.x += d0 / a.n; mn.y += d1 / a.n;
                s2.x += d0 * (xv[h].x - mn.x); s2.y += d1 * (xv[h].y - mn.y);
            }
            if (a.finish) {
                st2(scale + base + e, sqrt(a.c0 * (s2.x / a.nm1) + a.c1), sqrt(a.c0 * (s2.y / a.nm1) + a.c1), both);
                mn.x = mn.y = s2.x = s2.y = 0.0;
            }
            st2(mean + base + e, mn.x, mn.y, both);
            st2(m2 + base + e, s2.x, s2.y, both);
        }
    }
}

}  // namespace

extern "C" int qn_hmc_adapt(const double* cur, const double* alphas, int nmcmc, const int64_t* step_ptr, int parity, int C,
                            int64_t p, int m, double target_accept, int collect, int finish, int freeze, int n, double* da,
                            double* eps, double* mean, double* m2, double* scale, void* stream) {
    if (!alphas || !step_ptr || !da || !eps || C <= 0 || C > 65535 || p <= 0 || nmcmc < 1 || m < 1 ||
        (parity != 0 && parity != 1) || !(target_accept > 0.0 && target_accept < 1.0) ||
        (collect && (!cur || !mean || !m2 || n < 1)) || (finish && (!mean || !m2 || !scale || n < 2)) ||
        (finish && freeze)) {
        qn_set_error("qn_hmc_adapt: bad argument (collect needs cur / mean / m2 and n >= 1, finish needs scale and n >= 2, "
                     "finish and freeze exclude each other)");
        return QN_EINVAL;
    }
    const double t0 = 10.0, gamma = 0.05, kappa = 0.75;        // Stan's constants
    AdaptArgs a;
    a.nmcmc = nmcmc; a.par = parity; a.collect = collect ? 1 : 0; a.finish = finish ? 1 : 0; a.freeze = freeze ? 1 : 0;
    a.p = p;
    a.w = 1.0 / (m + t0); a.sg = std::sqrt((double)m) / gamma; a.eta = std::pow((double)m, -kappa); a.target = target_accept;
    a.n = n; a.nm1 = n - 1.0; a.c0 = n / (n + 5.0); a.c1 = 1e-3 * (5.0 / (n + 5.0));
    const int gx = (collect || finish) ? hmc_parts(p) : 1;
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_hmc_adapt, dim3(gx, C), dim3(HBLK), 0, static_cast<hipStream_t>(stream), a, cur, alphas, step_ptr,
                       da, eps, mean, m2, scale);
    QN_HIP_CHECK(hipGetLastError());
    return QN_OK;
}
