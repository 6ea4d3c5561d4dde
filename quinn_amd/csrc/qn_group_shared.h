// What the Gibbs-sampled priors share (qn_hyper.hip: the group precisions of the weights; qn_noise.hip: the noise level): the
// segment bounds of the weight groups in LDS, a row's per-group sums of squares in an order that depends on (p, seg) alone,
// and the bounded Marsaglia-Tsang Gamma draw.  Internal linkage, like qn_mcmc_shared.h: each translation unit gets its own
// copy.  FP contraction is switched off HERE, at file scope, for everything below and for the rest of the including file: the
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

// l.S[g] = sum of W[j]^2 over segment g, for every g < G, by the whole workgroup (HBLK threads); l.segs must be visible.
// Thread i adds the elements lo + i, lo + i + 256, ... into accumulator (k mod PUB) of round k; then a fixed tree.
__device__ __forceinline__ void group_sumsq(GroupLds& l, const double* __restrict__ W, int G) {
    for (int g = 0; g < G; ++g) {
        const int64_t lo = l.segs[g], hi = l.segs[g + 1];
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
        double v = (acc[0] + acc[1]) + (acc[2] + acc[3]);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if ((threadIdx.x & 63) == 0) l.red[g * 4 + (threadIdx.x >> 6)] = v;
    }
    __syncthreads();
    if (threadIdx.x < G) l.S[threadIdx.x] = (l.red[threadIdx.x * 4] + l.red[threadIdx.x * 4 + 1]) +
                                            (l.red[threadIdx.x * 4 + 2] + l.red[threadIdx.x * 4 + 3]);
    __syncthreads();
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
