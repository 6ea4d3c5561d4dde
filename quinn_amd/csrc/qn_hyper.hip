// Hierarchical Gaussian weight prior for the device HMC / MALA engines (build-only: the reference has no prior in NN_MCMC):
//   qn_prior_fold_g : qn_prior_fold with one precision per weight GROUP and per chain, read from device arrays (the one fold
//                     kernel and its three entry points are in qn_prior.hip)
//   qn_hyper_gibbs  : one exact Gibbs draw of every group's precision, and the refresh of the cached current state
// Groups g < G <= 32 are the contiguous segments [seg[g], seg[g + 1]) of the flat weight vector, n_g entries each:
//     w_j | tau_g ~ N(0, 1 / tau_g),   tau_g ~ Gamma(a0, rate b0),   tau_g | w ~ Gamma(a0 + n_g / 2, rate b0 + S_g / 2),
// S_g the group's sum of squares.  In the units of the sampler kernels (gs = -0.5 / sigma^2), per chain c,
//     lam[c, g] = sigma^2 tau[c, g],   c0[c] = sigma^2 (sum_g n_g log(2 pi / tau_g) - 2 log p(tau)),
//     sse' = sse + (sum_g lam_g S_g + c0),      g'_j = g_j + (2 lam_g(j)) w_j
// so gs sse' + (likelihood constants) is the JOINT log density of (w, tau) given the data, and the leapfrog, accept and adapt
// kernels run on it untouched (quinn_amd/mcmc/hyper.py restates everything here in numpy).
// The group of an element never comes from memory: a workgroup keeps the <= 33 segment bounds and the <= 32 factors in LDS,
// and a thread, whose elements only ever increase, keeps the bound of its current group and that group's factor in registers
// and walks forward when an element passes the bound.  Sums of squares: ONE workgroup sums a whole row group by group (a strided
// loop of its 256 threads over the segment, four accumulators per thread, a fixed tree), so the order of the additions
// depends on (p, seg) alone.  Plain vector loads and stores, no atomics, no fences, no arrival counters: whatever a launch
// reads and writes across a chain's workgroups (lam, c0, cur_lp, best_lp, the step counter) is double-buffered by a parity.
#include "qn_group_shared.h"

#pragma clang fp contract(off)

namespace {

constexpr int PURPOSE_GAMMA = 11;         // Philox purpose of the Gamma variates (qn_mcmc_shared.h)

// (GroupLds, load_segs, group_sumsq, group_map, gamma_draw and the Gibbs rounds' common part: qn_group_shared.h)

struct GibbsArgs : GibbsCommon {          // (opar: the parity of lam / c0)
    double sigma, a0, b0, kconst;         // kconst = a0 log b0 - lgamma(a0), the constant of one log p(tau_g)
};

// Every workgroup of a chain takes the whole decision itself -- the sums of squares of the chain's row and the G draws, from
// slot `opar` of lam / c0 and slot `par` of the scalars, which nobody writes in this launch -- then refreshes its own chunk of
// the cached gradient; workgroup 0 writes the other slots.
__global__ __launch_bounds__(HBLK) void k_hyper_gibbs(GibbsArgs a, const double* __restrict__ cur, double* __restrict__ gcur,
                                                      double* cur_lp, double* best_lp, double* __restrict__ lps, double* lam,
                                                      double* c0, const int64_t* __restrict__ seg, double* __restrict__ taus,
                                                      int64_t* step_ptr) {
    __shared__ GroupLds l;
    __shared__ double lamo[GMAX], lamn[GMAX], term[GMAX];
    const int b = blockIdx.y, G = a.G;
    const int64_t base = (int64_t)b * a.p;
    const int64_t t = step_ptr[a.par];
    const double* lo_ = lam + ((int64_t)a.opar * a.C + b) * G;
    load_segs(l, seg, G, a.p);
    if (threadIdx.x < G) lamo[threadIdx.x] = lo_[threadIdx.x];
    __syncthreads();
    group_sumsq(l, cur + base, G);
    const double s2 = a.sigma * a.sigma;
    if (threadIdx.x < G) {
        const int g = threadIdx.x;
        const double n = (double)(l.segs[g + 1] - l.segs[g]), S = l.S[g];
        double tau = NAN;
        if (fabs(S) < INFINITY)                                                // (finite; a sum of squares is never negative)
            tau = gamma_draw<PURPOSE_GAMMA>(a.seed, 2 * (uint64_t)t + 1, a.chain0 + b, g, a.a0 + 0.5 * n, a.b0 + 0.5 * S);
        const double ln = s2 * tau;
        lamn[g] = ln;
        l.fac[g] = 2.0 * (ln - lamo[g]);
        // this group's part of c0 / sigma^2: n_g log(2 pi / tau_g) - 2 log p(tau_g)
        const double lt = log(tau);
        term[g] = n * log(6.283185307179586 / tau) - 2.0 * (a.kconst + (a.a0 - 1.0) * lt - a.b0 * tau);
    }
    __syncthreads();
    bool ok = true;                       // every new precision positive and finite, in lam's units too, and its term finite
    for (int g = 0; g < G; ++g) ok = ok && lamn[g] > 0.0 && lamn[g] < INFINITY && fabs(term[g]) < INFINITY;
    // (two roundings: the product (2 (lam' - lam)) w, then the sum)
    if (ok) group_map<double>(l, cur + base, gcur + base, G, a.p, 0.0, [](double gv, double t_) { return gv + t_; });
    if (blockIdx.x != 0) return;
    double* ln_ = lam + ((int64_t)(1 - a.opar) * a.C + b) * G;
    if (threadIdx.x < G) {
        const int g = threadIdx.x;
        ln_[g] = ok ? lamn[g] : lamo[g];
        if (taus) {
            double* row = taus + ((int64_t)b * (a.nrounds + 1) + a.round) * G;
            row[G + g] = ok ? lamn[g] / s2 : row[g];                            // (a frozen chain repeats its last column)
        }
    }
    if (threadIdx.x == 0) {
        const double c0o = c0[a.opar * a.C + b], clp = cur_lp[a.par * a.C + b];
        double nlp = clp, c0n = c0o;
        if (ok) {
            double dsum = (lamn[0] - lamo[0]) * l.S[0], tsum = term[0];
            for (int g = 1; g < G; ++g) {
                dsum = dsum + (lamn[g] - lamo[g]) * l.S[g];
                tsum = tsum + term[g];
            }
            c0n = s2 * tsum;
            nlp = clp + (-0.5 / s2) * (dsum + (c0n - c0o));
        }
        c0[(1 - a.opar) * a.C + b] = c0n;
        gibbs_other_slot(a, b, t, ok, nlp, cur_lp, best_lp, lps, step_ptr);
    }
}

}  // namespace

extern "C" int qn_hyper_gibbs(const double* cur, double* grad_cur, double* cur_lp, double* best_lp, double* lps, double* lam,
                              double* c0, const int64_t* seg, double* taus, int64_t* step_ptr, double sigma, double a0,
                              double b0, int G, int round, int nrounds, int C, int chain0, int64_t p, int nmcmc, uint64_t seed,
                              int parity, int hyper_parity, void* stream) {
    GibbsArgs a;
    a.G = G; a.round = round; a.nrounds = nrounds; a.C = C; a.chain0 = chain0; a.nmcmc = nmcmc; a.par = parity; a.opar = hyper_parity;
    a.p = p; a.seed = seed; a.sigma = sigma; a.a0 = a0; a.b0 = b0;
    if (!gibbs_sizes_ok("qn_hyper_gibbs", 1, a, sigma, a0, b0) || !gibbs_round_ok("qn_hyper_gibbs", "hyper_parity", a))
        return QN_EINVAL;
    if (!cur || !grad_cur || !cur_lp || !best_lp || !lps || !lam || !c0 || !seg || !step_ptr) {
        qn_set_error("qn_hyper_gibbs: a required pointer is NULL (only taus is optional)");
        return QN_EINVAL;
    }
    a.kconst = a0 * std::log(b0) - std::lgamma(a0);
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_hyper_gibbs, dim3(hmc_parts(p), C), dim3(HBLK), 0, static_cast<hipStream_t>(stream), a, cur, grad_cur,
                       cur_lp, best_lp, lps, lam, c0, seg, taus, step_ptr);
    QN_HIP_CHECK(hipGetLastError());
    return QN_OK;
}
