// Isotropic Gaussian weight prior N(0, priorsigma^2 I) for the device samplers, folded into what the forward / gradient
// kernels return (build-only: the reference has no prior in NN_MCMC).  Every device engine turns a bare SSE and d SSE / d W into
// log-posteriors and forces with gs = -0.5 / sigma^2, so in those units, with lam = sigma^2 / priorsigma^2 and
// c0 = sigma^2 p log(2 pi priorsigma^2),
//     sse' = sse + (lam |w|^2 + c0)      ->  gs sse' = gs sse + log N(w; 0, priorsigma^2 I)
//     g'   = g + (2 lam) w               ->  gs g'   = gs g - w / priorsigma^2
// and one qn_prior_fold launch behind a forward / gradient call hands every accept, leapfrog, adapt, swap and SG kernel the
// posterior with the prior, their code untouched.
// Gradient: elementwise, the element -> thread map of k_hmc_leap; every entry is formed in float64 with one rounding per
// operation (FP contraction is off for the whole file: hipcc would fuse the product into the sum), a float32 gradient is
// widened, updated and rounded once.  Sum of squares: workgroup 0 of every chain sums the WHOLE row itself (a strided loop of
// its 256 threads, four accumulators per thread, block_sum_256), so the order of the additions depends on p alone -- not on the
// grid, not on C, not on the chain's place in the launch -- and it is the only writer of the chain's SSE entry.  Plain vector
// loads and stores, no atomics, no fences: two calls on equal inputs give equal bits.  A row is 68 KB at cfg2 (p = 8513).
#include "qn_mcmc_shared.h"

#pragma clang fp contract(off)

namespace {

constexpr int PUB = 4;                    // independent accumulators (and loads in flight) per thread of the row sum

template <typename TG>
__global__ __launch_bounds__(HBLK) void k_prior_fold(const double* __restrict__ W, double lam, double two_lam, double c0,
                                                     TG* __restrict__ g, double* __restrict__ sse, int sse_stride, int64_t p) {
    __shared__ double red[4];
    const int b = blockIdx.y;
    const int64_t base = (int64_t)b * p;
    if (g) {
        const int64_t chunk = (p + gridDim.x - 1) / gridDim.x;
        const int64_t lo = blockIdx.x * chunk, hi = lo + chunk < p ? lo + chunk : p;
        for (int64_t e0 = lo + threadIdx.x; e0 < hi; e0 += (int64_t)HUB * HBLK) {
            double gv[HUB], wv[HUB];
#pragma unroll
            for (int u = 0; u < HUB; ++u) {
                const int64_t e = e0 + (int64_t)u * HBLK;
                const bool in = e < hi;
                gv[u] = in ? (double)g[base + e] : 0.0;
                wv[u] = in ? W[base + e] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < HUB; ++u) {
                const int64_t e = e0 + (int64_t)u * HBLK;
                if (e >= hi) break;
                const double t = two_lam * wv[u];                       // (two roundings: the product, then the sum)
                g[base + e] = (TG)(gv[u] + t);
            }
        }
    }
    if (!sse || blockIdx.x != 0) return;                               // (uniform over the workgroup)
    // the whole row, whatever the grid: thread i adds the elements i, i + 256, ... into accumulator (k mod PUB) of round k
    double acc[PUB];
#pragma unroll
    for (int u = 0; u < PUB; ++u) acc[u] = 0.0;
    for (int64_t e0 = threadIdx.x; e0 < p; e0 += (int64_t)PUB * HBLK) {
        double wv[PUB];
#pragma unroll
        for (int u = 0; u < PUB; ++u) {
            const int64_t e = e0 + (int64_t)u * HBLK;
            wv[u] = e < p ? W[base + e] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < PUB; ++u) acc[u] = acc[u] + wv[u] * wv[u];
    }
    const double tot = block_sum_256((acc[0] + acc[1]) + (acc[2] + acc[3]), red);
    if (threadIdx.x == 0) {
        double* out = sse + (int64_t)b * sse_stride;
        const double term = lam * tot + c0;
        *out = *out + term;
    }
}

}  // namespace

extern "C" int qn_prior_fold(const double* W, double lam, double c0, void* grad, int gdtype, double* sse, int sse_stride, int C,
                             int64_t p, void* stream) {
    if (!W) {
        qn_set_error("qn_prior_fold: W is NULL");
        return QN_EINVAL;
    }
    if (!grad && !sse) {
        qn_set_error("qn_prior_fold: grad and sse are both NULL (nothing to fold the prior into)");
        return QN_EINVAL;
    }
    if (!(lam > 0.0) || !std::isfinite(lam) || !std::isfinite(c0)) {
        qn_set_error("qn_prior_fold: lam = %g must be > 0 and finite, c0 = %g finite", lam, c0);
        return QN_EINVAL;
    }
    if (C < 1 || C > 65535 || p < 1) {
        qn_set_error("qn_prior_fold: bad size (1 <= C = %d <= 65535, p = %lld >= 1)", C, (long long)p);
        return QN_EINVAL;
    }
    if (sse && sse_stride < 1) {
        qn_set_error("qn_prior_fold: sse_stride = %d must be >= 1", sse_stride);
        return QN_EINVAL;
    }
    if (grad && gdtype != QN_F64 && gdtype != QN_F32) {
        qn_set_error("qn_prior_fold: gdtype = %d is neither QN_F64 nor QN_F32", gdtype);
        return QN_EINVAL;
    }
    const dim3 grid(grad ? hmc_parts(p) : 1, C), blk(HBLK);
    const double two_lam = 2.0 * lam;
    hipStream_t st = static_cast<hipStream_t>(stream);
    (void)hipGetLastError();
    if (grad && gdtype == QN_F32)
        hipLaunchKernelGGL(k_prior_fold<float>, grid, blk, 0, st, W, lam, two_lam, c0, static_cast<float*>(grad), sse, sse_stride, p);
    else
        hipLaunchKernelGGL(k_prior_fold<double>, grid, blk, 0, st, W, lam, two_lam, c0, static_cast<double*>(grad), sse, sse_stride, p);
    QN_HIP_CHECK(hipGetLastError());
    return QN_OK;
}
