// What the fold kernel (qn_prior.hip) and the Gibbs rounds (qn_hyper.hip: the group precisions of the weights; qn_noise.hip: the
// noise level) share: the segment bounds of the weight groups in LDS, a row's per-group sums of squares in an order that
// depends on (p, seg) alone, the one elementwise pass over a row and the prior's part of a folded SSE, the bounded
// Marsaglia-Tsang Gamma draw, and what the two Gibbs entry points check and write alike.  Internal linkage, like
// qn_mcmc_shared.h: each translation unit gets its own copy.  FP contraction is switched off HERE, at file scope, for everything below and for the rest of the including file: the
// sums and the draw are one rounding per operation, as they were when they stood below qn_hyper.hip's own pragma.
#pragma once
#include "qn_mcmc_shared.h"

#pragma clang fp contract(off)

namespace {

constexpr int GMAX = 32;                  // groups at most
constexpr int PUB = 4;                    // independent accumulators (and loads in flight) per thread of a segment's sum
constexpr int GAMMA_TRIES = 64;           // bound of the rejection loop

struct GroupLds {
    int64_t segs[GMAX + 1];               // the segment bounds, clamped to [0, p]
    double fac[GMAX];                     // the per-group factor of the elementwise pass (2 lam, or 2 (lam' - lam))
    double S[GMAX];                       // the per-group sums of squares
    double red[GMAX * 4];                 // one partial per group and wave
};

// segment bounds -> LDS, clamped: no bound can take an index out of [0, p], whatever the array holds
__device__ __forceinline__ void load_segs(GroupLds& l, const int64_t* __restrict__ seg, int G, int64_t p) {
    if (threadIdx.x <= G) {
        int64_t v = seg[threadIdx.x];
        v = v < 0 ? 0 : (v > p ? p : v);
        l.segs[threadIdx.x] = threadIdx.x == 0 ? 0 : (threadIdx.x == G ? p : v);
    }
}

// this thread's part of the sum of W[j]^2 over [lo, hi), the whole workgroup (HBLK threads) at work: thread i adds the elements
// lo + i, lo + i + 256, ... into accumulator (k mod PUB) of round k, then (a0 + a1) + (a2 + a3).
__device__ __forceinline__ double segment_sumsq(const double* __restrict__ W, int64_t lo, int64_t hi) {
    double acc[PUB];
#pragma unroll
    for (int u = 0; u < PUB; ++u) acc[u] = 0.0;
    for (int64_t e0 = lo + threadIdx.x; e0 < hi; e0 += (int64_t)PUB * HBLK) {
        double wv[PUB];
#pragma unroll
        for (int u = 0; u < PUB; ++u) {
            const int64_t e = e0 + (int64_t)u * HBLK;
            wv[u] = e < hi ? W[e] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < PUB; ++u) acc[u] = acc[u] + wv[u] * wv[u];
    }
    return (acc[0] + acc[1]) + (acc[2] + acc[3]);
}

// l.S[g] = sum of W[j]^2 over segment g, for every g < G, by the whole workgroup; l.segs must be visible.  The tree of
// block_sum_256 per group (wave shuffles, then the four wave partials as (r0 + r1) + (r2 + r3)) with ONE barrier for all groups.
__device__ __forceinline__ void group_sumsq(GroupLds& l, const double* __restrict__ W, int G) {
    for (int g = 0; g < G; ++g) {
        double v = segment_sumsq(W, l.segs[g], l.segs[g + 1]);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if ((threadIdx.x & 63) == 0) l.red[g * 4 + (threadIdx.x >> 6)] = v;
    }
    __syncthreads();
    if (threadIdx.x < G) l.S[threadIdx.x] = (l.red[threadIdx.x * 4] + l.red[threadIdx.x * 4 + 1]) +
                                            (l.red[threadIdx.x * 4 + 2] + l.red[threadIdx.x * 4 + 3]);
    __syncthreads();
}

// g[e] <- op(g[e], fac[group of e] * W[e]) over this workgroup's chunk of the row (W, g: the row's first element): the grid and
// the element -> thread map of k_hmc_leap; a thread's elements only increase, so it keeps the bound of its current group and
// that group's factor in registers and walks forward in LDS when an element passes the bound.  Everything is formed in float64,
// one rounding per operation, and TG is rounded once.  G = 0: ONE group [0, p) with the factor f0, and l is not read.
template <typename TG, typename OP>
__device__ __forceinline__ void group_map(const GroupLds& l, const double* __restrict__ W, TG* __restrict__ g, int G, int64_t p,
                                          double f0, OP op) {
    const int64_t chunk = (p + gridDim.x - 1) / gridDim.x;
    const int64_t lo = blockIdx.x * chunk, hi = lo + chunk < p ? lo + chunk : p;
    int gi = 0;
    int64_t nxt = G > 0 ? l.segs[1] : p;                                   // the end of the thread's current group
    double f = G > 0 ? l.fac[0] : f0;
    for (int64_t e0 = lo + threadIdx.x; e0 < hi; e0 += (int64_t)HUB * HBLK) {
        double gv[HUB], wv[HUB];
#pragma unroll
        for (int u = 0; u < HUB; ++u) {
            const int64_t e = e0 + (int64_t)u * HBLK;
            const bool in = e < hi;
            gv[u] = in ? (double)g[e] : 0.0;
            wv[u] = in ? W[e] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < HUB; ++u) {
            const int64_t e = e0 + (int64_t)u * HBLK;
            if (e >= hi) break;
            while (e >= nxt && gi + 1 < G) {                                // (elements only increase: a forward walk in LDS)
                ++gi;
                nxt = l.segs[gi + 1];
                f = l.fac[gi];
            }
            g[e] = (TG)op(gv[u], f * wv[u]);
        }
    }
}

// the prior's part of a folded SSE: the terms lam_g S_g left to right, then c0 (G >= 1; l.S from group_sumsq)
__device__ __forceinline__ double prior_term(const GroupLds& l, const double* __restrict__ lam, double c0, int G) {
    double term = lam[0] * l.S[0];
    for (int k = 1; k < G; ++k) term = term + lam[k] * l.S[k];
    return term + c0;
}

// ---- what qn_hyper_gibbs and qn_noise_gibbs take, check and write alike
struct GibbsCommon {
    int G, round, nrounds, C, chain0, nmcmc, par, opar;                    // opar: the parity of the round's own arrays
    int64_t p;
    uint64_t seed;
};

// the refusals both entry points make, in two parts (qn_noise_gibbs has a check of its own between them); gmin: the fewest
// groups, oname: what the caller calls `opar`
inline bool gibbs_sizes_ok(const char* fn, int gmin, const GibbsCommon& a, double sigma, double a0, double b0) {
    if (!(a0 > 0.0) || !std::isfinite(a0) || !(b0 > 0.0) || !std::isfinite(b0) || !(sigma > 0.0) || !std::isfinite(sigma))
        qn_set_error("%s: a0 = %g, b0 = %g and sigma = %g must be > 0 and finite", fn, a0, b0, sigma);
    else if (a.G < gmin || a.G > GMAX)
        qn_set_error("%s: G = %d groups, %d <= G <= %d", fn, a.G, gmin, GMAX);
    else if (a.C < 1 || a.C > 65535 || a.p < 1 || a.p < a.G || a.chain0 < 0 || a.nmcmc < 1)
        qn_set_error("%s: bad size (1 <= C = %d <= 65535, p = %lld >= max(1, G = %d), chain0 = %d >= 0, nmcmc = %d >= 1)", fn,
                     a.C, (long long)a.p, a.G, a.chain0, a.nmcmc);
    else
        return true;
    return false;
}
inline bool gibbs_round_ok(const char* fn, const char* oname, const GibbsCommon& a) {
    if (a.nrounds < 1 || a.round < 0 || a.round >= a.nrounds)
        qn_set_error("%s: round = %d outside 0 .. nrounds - 1 = %d", fn, a.round, a.nrounds - 1);
    else if ((a.par != 0 && a.par != 1) || (a.opar != 0 && a.opar != 1))
        qn_set_error("%s: parity = %d and %s = %d are 0 or 1", fn, a.par, oname, a.opar);
    else
        return true;
    return false;
}

// chain b's scalars after a round, by one thread: the other slot of cur_lp / best_lp, the stored trace, the step counter
__device__ __forceinline__ void gibbs_other_slot(const GibbsCommon& a, int b, int64_t t, bool ok, double nlp, double* cur_lp,
                                                 double* best_lp, double* __restrict__ lps, int64_t* step_ptr) {
    const int so = a.par * a.C, sn = (1 - a.par) * a.C;
    cur_lp[sn + b] = nlp;
    best_lp[sn + b] = best_lp[so + b];
    // the stored trace is that of the state step t + 1 starts from (the convention of qn_pt_swap)
    if (ok && t >= 0 && t <= a.nmcmc) lps[(int64_t)b * (a.nmcmc + 1) + t] = nlp;
    if (b == 0) step_ptr[1 - a.par] = t;                                   // no step was taken: the caller only flips its parity
}

// ---- Gamma(shape, rate) by Marsaglia & Tsang (2000), the log test only (no squeeze), at most GAMMA_TRIES attempts, from the
// Philox purpose PURPOSE.  Attempt k of variate g reads two Philox blocks, index (g << 16) | (k << 4) | block: block 0 gives the
// normal (Box-Muller in float64 on u01(words 0, 1), u01(words 2, 3)), block 1 the uniform of the test (words 0, 1).  shape < 1:
// the draw at shape + 1 times u^(1 / shape), u from words 0, 1 of index (g << 16) | (GAMMA_TRIES << 4).  No attempt accepted:
// shape / rate.
template <int PURPOSE>
__device__ double gamma_draw(uint64_t seed, uint64_t stream, int chain, int g, double shape, double rate) {
    const double a = shape < 1.0 ? shape + 1.0 : shape;
    const double d = a - 1.0 / 3.0, c = 1.0 / sqrt(9.0 * d);
    Philox ph;
    for (int k = 0; k < GAMMA_TRIES; ++k) {
        ph.gen(seed, stream, ctr_of(chain, PURPOSE, ((uint64_t)g << 16) | ((uint64_t)k << 4)));
        const double u1 = u01(ph.c[0], ph.c[1]), u2 = u01(ph.c[2], ph.c[3]);
        const double x = sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2);
        const double t = 1.0 + c * x;
        if (!(t > 0.0)) continue;
        const double v = t * t * t;
        ph.gen(seed, stream, ctr_of(chain, PURPOSE, ((uint64_t)g << 16) | ((uint64_t)k << 4) | 1));
        const double u = u01(ph.c[0], ph.c[1]);
        if (log(u) < 0.5 * x * x + d - d * v + d * log(v)) {
            double gam = d * v;
            if (shape < 1.0) {
                ph.gen(seed, stream, ctr_of(chain, PURPOSE, ((uint64_t)g << 16) | ((uint64_t)GAMMA_TRIES << 4)));
                gam = gam * exp(log(u01(ph.c[0], ph.c[1])) / shape);
            }
            return gam / rate;
        }
    }
    return shape / rate;
}

}  // namespace
