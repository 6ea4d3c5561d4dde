// Conjugate hyper-prior on the noise level of the Gaussian likelihood for the device HMC / MALA engines (build-only: the
// reference's noise level is a hand-set scalar):
//   qn_noise_fold  : the per-chain noise level AND the weight prior (none, scalar or per group) folded into a gradient call's
//                    outputs in ONE launch; it stands where qn_prior_fold / qn_prior_fold_g stand (the one fold kernel and
//                    its three entry points are in qn_prior.hip)
//   qn_noise_gibbs : one exact Gibbs draw of every chain's noise precision, and the refresh of the cached current state
// One variance s2_c per chain, shared by all n = N * o entries of y:
//     y_k | w, s2 ~ N(M_w(x)_k, s2),   1 / s2 ~ Gamma(a0, rate b0),   1 / s2 | w, y ~ Gamma(a0 + n / 2, rate b0 + SSE(w) / 2).
// The sampler kernels keep the NOMINAL sigma0 (gs = -0.5 / sigma0^2, their constant (N / 2) log 2 pi + N log sigma0); per chain
//     kappa = sigma0^2 / s2,      d0 = sigma0^2 (n log(2 pi s2) - 2 log p(s2) - N log(2 pi sigma0^2)),
//     sse'  = kappa sse + (sum_g lam_g S_g + c0) + d0,      g'_j = kappa g_j + (2 lam_g(j)) w_j
// so gs sse' - (their constant) is the JOINT log density of (w, s2[, tau]) given the data, and the leapfrog, accept and adapt
// kernels run on it untouched (quinn_amd/mcmc/noise.py restates everything here in numpy).
// The Gibbs round needs no state of its own: the data SSE of the current state is recovered by inverting the fold from the
// cached log density.  Plain vector loads and stores, no atomics, no fences, no arrival counters: whatever a launch reads and
// writes across a chain's workgroups (kappa, d0, cur_lp, best_lp, the step counter) is double-buffered by a parity.
#include "qn_group_shared.h"

#pragma clang fp contract(off)

namespace {

constexpr int PURPOSE_NOISE = 12;         // Philox purpose of the noise precision's Gamma variate (qn_mcmc_shared.h)

// (GroupLds, load_segs, group_sumsq, group_map, prior_term, gamma_draw and the Gibbs rounds' common part: qn_group_shared.h)

struct NoiseArgs : GibbsCommon {          // (opar: the parity of kappa / d0)
    // s0sq = sigma0^2, h = 0.5 / sigma0^2, lik_const = (N / 2) log 2 pi + N log sigma0 (the accept kernel's), n = N * o,
    // nlog0 = N log(2 pi sigma0^2), kconst = a0 log b0 - lgamma(a0)
    double s0sq, h, lik_const, n, nlog0, a0, b0, kconst;
};

// Every workgroup of a chain takes the whole decision itself -- the prior's part of the cached density from the chain's row,
// the recovered SSE, the draw, the new constants -- from slot `opar` of kappa / d0, slot `par` of the scalars and the current
// lam / c0, which nobody writes in this launch; then it refreshes its own chunk of the cached gradient; workgroup 0 writes the
// other slots.
__global__ __launch_bounds__(HBLK) void k_noise_gibbs(NoiseArgs a, const double* __restrict__ cur, double* __restrict__ gcur,
                                                      double* cur_lp, double* best_lp, double* __restrict__ lps, double* kappa,
                                                      double* d0, const double* __restrict__ lam, const double* __restrict__ c0,
                                                      const int64_t* __restrict__ seg, double* __restrict__ sig,
                                                      double* __restrict__ sse_rec, int64_t* step_ptr) {
    __shared__ GroupLds l;
    __shared__ double dec[6];                                              // ok, kappa', d0', sse, s2', r - 1
    const int b = blockIdx.y, G = a.G;
    const int64_t base = (int64_t)b * a.p;
    const int64_t t = step_ptr[a.par];
    if (G > 0) {
        load_segs(l, seg, G, a.p);
        if (threadIdx.x < G) l.fac[threadIdx.x] = 2.0 * lam[(int64_t)b * G + threadIdx.x];
        __syncthreads();
        group_sumsq(l, cur + base, G);
    }
    const double ko = kappa[a.opar * a.C + b], d0o = d0[a.opar * a.C + b], clp = cur_lp[a.par * a.C + b];
    if (threadIdx.x == 0) {
        // the data SSE of the current state: the fold inverted, in this order
        const double F = (-clp - a.lik_const) / a.h;
        double sse = F - d0o;
        if (G > 0) sse = sse - prior_term(l, lam + (int64_t)b * G, c0[b], G);
        sse = sse / ko;
        double kn = NAN, d0n = NAN, s2n = NAN;
        if (fabs(sse) < INFINITY && sse >= 0.0) {
            const double prec = gamma_draw<PURPOSE_NOISE>(a.seed, 2 * (uint64_t)t + 1, a.chain0 + b, 0, a.a0 + 0.5 * a.n,
                                                          a.b0 + 0.5 * sse);
            s2n = 1.0 / prec;
            kn = a.s0sq / s2n;
            const double lp = a.kconst + (a.a0 + 1.0) * log(1.0 / s2n) - a.b0 / s2n;
            d0n = a.s0sq * ((a.n * log(6.283185307179586 * s2n) - 2.0 * lp) - a.nlog0);
        }
        const bool ok = kn > 0.0 && kn < INFINITY && s2n > 0.0 && s2n < INFINITY && fabs(d0n) < INFINITY;
        dec[0] = ok ? 1.0 : 0.0;
        dec[1] = kn;
        dec[2] = d0n;
        dec[3] = sse;
        dec[4] = s2n;
        dec[5] = kn / ko - 1.0;
    }
    __syncthreads();
    const bool ok = dec[0] != 0.0;
    if (ok) {
        // grad_cur + (r - 1) (grad_cur - (2 lam) w): the likelihood's part of the cached gradient rescaled, the prior's kept
        const double rm1 = dec[5];
        if (G > 0) group_map<double>(l, cur + base, gcur + base, G, a.p, 0.0, [rm1](double gv, double t_) { return gv + rm1 * (gv - t_); });
        else group_map<double>(l, cur + base, gcur + base, G, a.p, 0.0, [rm1](double gv, double) { return gv + rm1 * gv; });
    }
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const int no = (1 - a.opar) * a.C;
    double nlp = clp;
    if (ok) nlp = clp - a.h * ((dec[1] - ko) * dec[3] + (dec[2] - d0o));
    kappa[no + b] = ok ? dec[1] : ko;
    d0[no + b] = ok ? dec[2] : d0o;
    if (sse_rec) sse_rec[b] = dec[3];                                          // (whatever the decision: what the inversion gave)
    if (sig) {
        double* row = sig + (int64_t)b * (a.nrounds + 1) + a.round;
        row[1] = ok ? sqrt(dec[4]) : row[0];                                   // (a frozen chain repeats its last column)
    }
    gibbs_other_slot(a, b, t, ok, nlp, cur_lp, best_lp, lps, step_ptr);
}

}  // namespace

extern "C" int qn_noise_gibbs(const double* cur, double* grad_cur, double* cur_lp, double* best_lp, double* lps, double* kappa,
                              double* d0, const double* lam, const double* c0, const int64_t* seg, double* sig,
                              double* sse_rec, int64_t* step_ptr, double sigma, double a0, double b0, int n_rows, int64_t n, int G, int round,
                              int nrounds, int C, int chain0, int64_t p, int nmcmc, uint64_t seed, int parity, int noise_parity,
                              void* stream) {
    NoiseArgs a;
    a.G = G; a.round = round; a.nrounds = nrounds; a.C = C; a.chain0 = chain0; a.nmcmc = nmcmc; a.par = parity; a.opar = noise_parity;
    a.p = p; a.seed = seed; a.a0 = a0; a.b0 = b0; a.n = (double)n;
    if (!gibbs_sizes_ok("qn_noise_gibbs", 0, a, sigma, a0, b0)) return QN_EINVAL;
    if (n_rows < 1 || n < n_rows) {
        qn_set_error("qn_noise_gibbs: n_rows = %d >= 1 rows and n = %lld >= n_rows entries of y", n_rows, (long long)n);
        return QN_EINVAL;
    }
    if (!gibbs_round_ok("qn_noise_gibbs", "noise_parity", a)) return QN_EINVAL;
    if (!cur || !grad_cur || !cur_lp || !best_lp || !lps || !kappa || !d0 || !step_ptr) {
        qn_set_error("qn_noise_gibbs: a required pointer is NULL (only sig and sse_rec are optional, and lam, c0, seg with G = 0)");
        return QN_EINVAL;
    }
    if (G > 0 && (!lam || !c0 || !seg)) {
        qn_set_error("qn_noise_gibbs: lam, c0 or seg is NULL with G = %d groups (G = 0: no weight prior)", G);
        return QN_EINVAL;
    }
    a.s0sq = sigma * sigma;
    a.h = 0.5 / a.s0sq;
    a.lik_const = 0.5 * n_rows * std::log(2.0 * M_PI) + n_rows * std::log(sigma);
    a.nlog0 = n_rows * std::log(6.283185307179586 * a.s0sq);
    a.kconst = a0 * std::log(b0) - std::lgamma(a0);
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_noise_gibbs, dim3(hmc_parts(p), C), dim3(HBLK), 0, static_cast<hipStream_t>(stream), a, cur, grad_cur,
                       cur_lp, best_lp, lps, kappa, d0, lam, c0, seg, sig, sse_rec, step_ptr);
    QN_HIP_CHECK(hipGetLastError());
    return QN_OK;
}
