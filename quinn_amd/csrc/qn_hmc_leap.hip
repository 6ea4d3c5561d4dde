// The leapfrog of the device HMC / MALA engines: ONE begin kernel and ONE leap kernel behind all six entry points
//   qn_hmc_begin   / qn_hmc_leap   : a fixed step size, passed by value
//   qn_hmc_begin_s / qn_hmc_leap_s : a per-chain step size eps [C] and an optional per-parameter scale [C, p] (square root of
//                                    the inverse diagonal mass) on the device; warm-up: qn_hmc_adapt.hip
//   qn_hmc_begin_t / qn_hmc_leap_t : the same with a per-chain inverse temperature beta [C]: chain c samples pi^beta_c;
//                                    replica exchange: qn_temper.hip
// The accept calls (qn_hmc_accept, qn_hmc_accept_t) are in qn_mcmc.hip, next to the kernel they share with plain Metropolis.
// The leapfrog runs in whitened momenta u = s * r (r the momentum, M^-1 = diag(s^2)): u ~ N(0, I), K = |u|^2 / 2, a kick is
// u += (f eps_c gs_c) s * d SSE, a drift q += eps_c s * u, with gs_c = gs * beta_c (gs = -0.5 / sigma^2: d logpost = gs * d SSE),
// so the force is beta_c * d logpost and drifts do not see beta.  What an entry point does not have is a compile-time choice
// (TE, HS, HB below) and leaves no instruction behind: s = 1 and beta_c = 1 are exact, so every entry point computes the same
// bits from the same numbers -- same grid, same element -> thread map, same Philox keys, same fixed-order partial sums -- and
// qn_hmc_accept serves them all.  HBM-bound elementwise work; all stores are ordinary vector stores, no atomics, no fences.
#include "qn_mcmc_shared.h"
#include <type_traits>

namespace {

// TE, where a chain's step size comes from: `double`, the fixed step as a kernel argument (no device array is read, none
// exists), or `const double*`, eps [C] on the device.
__device__ __forceinline__ double eps_of(double eps, int) { return eps; }
__device__ __forceinline__ double eps_of(const double* eps, int b) { return eps[b]; }
inline bool eps_missing(double) { return false; }
inline bool eps_missing(const double* eps) { return !eps; }

// momentum z ~ N(0, I) (Philox stream 2 * step, keyed by the global chain id), half kick with the cached gradient of the
// current state, first drift:
//   mom = z + (hk_c s) g_cur;  q = cur + (eps_c s) mom;  K_cur partial = sum z^2                  (hk_c = (eps_c / 2) gs_c)
// One Philox block = one PAIR of consecutive elements = one 16-byte access per array (8-byte aligned: rows of odd length).
// HS: a scale array is given; HB: beta is given.
template <typename TE, bool HS, bool HB>
__global__ __launch_bounds__(HBLK) void k_hmc_begin(const double* __restrict__ cur, const double* __restrict__ gcur, TE eps,
                                                    const double* __restrict__ scale, const double* __restrict__ beta,
                                                    double gs, int chain0, int64_t p, uint64_t seed,
                                                    const int64_t* __restrict__ step_ptr, double* __restrict__ mom,
                                                    double* __restrict__ q, double* __restrict__ kin_parts) {
    __shared__ double red[4];
    const int b = blockIdx.y;
    const uint64_t step = (uint64_t)*step_ptr;
    const double eps_c = eps_of(eps, b);
    if (HB) gs = gs * beta[b];
    const double half_kick = 0.5 * eps_c * gs;
    const int64_t base = (int64_t)b * p;
    const int64_t npair = (p + 1) / 2;
    const int64_t pchunk = (npair + gridDim.x - 1) / gridDim.x;
    const int64_t lo = blockIdx.x * pchunk, hi = lo + pchunk < npair ? lo + pchunk : npair;
    double ss = 0.0;
    for (int64_t j = lo + threadIdx.x; j < hi; j += HBLK) {
        Philox ph;
        ph.gen(seed, 2 * step, ctr_of(chain0 + b, 0, (uint64_t)j));
        double za, zb;
        normal2(ph, za, zb);
        const int64_t e = 2 * j;
        const bool both = e + 1 < p;
        const d2u one = {1.0, 1.0};
        const d2u gv = ld2(gcur + base + e, both), cv = ld2(cur + base + e, both);
        const d2u sv = HS ? ld2(scale + base + e, both) : one;
        const double m0 = fma(half_kick * sv.x, gv.x, za);
        const double q0 = fma(eps_c * sv.x, m0, cv.x);
        ss = fma(za, za, ss);
        double m1 = 0.0, q1 = 0.0;
        if (both) {
            m1 = fma(half_kick * sv.y, gv.y, zb);
            q1 = fma(eps_c * sv.y, m1, cv.y);
            ss = fma(zb, zb, ss);
        }
        st2(mom + base + e, m0, m1, both);
        st2(q + base + e, q0, q1, both);
    }
    const double tot = block_sum_256(ss, red);
    if (threadIdx.x == 0) kin_parts[(int64_t)b * gridDim.x + blockIdx.x] = tot;
}

// kick with the gradient at q (TG: float64 or float32), then (inner step) drift, or (last step) the proposal's kinetic energy:
//   mom += (kick_c s) g;   last ? K_prop partial = sum mom^2 : q += (eps_c s) mom                 (kick_c = f eps_c gs_c, f = 1 or 1/2)
// HS is a compile-time choice so that the unrolled loads carry no per-element branch.
template <typename TG, typename TE, bool HS, bool HB>
__global__ __launch_bounds__(HBLK) void k_hmc_leap(const TG* __restrict__ g, TE eps, const double* __restrict__ scale,
                                                   const double* __restrict__ beta, double f, double gs, int last, int64_t p,
                                                   double* __restrict__ mom, double* __restrict__ q,
                                                   double* __restrict__ kin_parts) {
    __shared__ double red[4];
    const int b = blockIdx.y;
    const double eps_c = eps_of(eps, b);
    if (HB) gs = gs * beta[b];
    const double kick = f * eps_c * gs;
    const int64_t base = (int64_t)b * p;
    const int64_t chunk = (p + gridDim.x - 1) / gridDim.x;
    const int64_t lo = blockIdx.x * chunk, hi = lo + chunk < p ? lo + chunk : p;
    double ss = 0.0;
    for (int64_t e0 = lo + threadIdx.x; e0 < hi; e0 += (int64_t)HUB * HBLK) {
        double gv[HUB], mv[HUB], qv[HUB], sv[HUB];
#pragma unroll
        for (int u = 0; u < HUB; ++u) {
            const int64_t e = e0 + (int64_t)u * HBLK;
            const bool in = e < hi;
            gv[u] = in ? (double)g[base + e] : 0.0;
            mv[u] = in ? mom[base + e] : 0.0;
            qv[u] = (in && !last) ? q[base + e] : 0.0;
            sv[u] = (HS && in) ? scale[base + e] : 1.0;
        }
#pragma unroll
        for (int u = 0; u < HUB; ++u) {
            const int64_t e = e0 + (int64_t)u * HBLK;
            if (e >= hi) break;
            const double m = fma(kick * sv[u], gv[u], mv[u]);
            mom[base + e] = m;
            if (last) ss = fma(m, m, ss);
            else q[base + e] = fma(eps_c * sv[u], m, qv[u]);
        }
    }
    if (last) {
        const double tot = block_sum_256(ss, red);
        if (threadIdx.x == 0) kin_parts[(int64_t)b * gridDim.x + blockIdx.x] = tot;
    }
}

// go(HS, HB) with the two flags as compile-time constants.  A fixed step has neither array: one instantiation.
template <typename TE, typename F>
void with_flags(const double* scale, const double* beta, F go) {
    using Y = std::true_type;
    using N = std::false_type;
    if constexpr (!std::is_pointer<TE>::value) go(N{}, N{});
    else if (scale && beta) go(Y{}, Y{});
    else if (scale) go(Y{}, N{});
    else if (beta) go(N{}, Y{});
    else go(N{}, N{});
}

// The one checked launch of each phase; `who` is the entry point that was called.
template <typename TE>
int hmc_begin_launch(const char* who, const double* cur, const double* grad_cur, double sigma, TE eps, const double* scale,
                     const double* beta, int C, int chain0, int64_t p, uint64_t seed, const int64_t* step_ptr, double* mom,
                     double* q, double* kin_cur_parts, void* stream) {
    if (!cur || !grad_cur || eps_missing(eps) || !step_ptr || !mom || !q || !kin_cur_parts || C <= 0 || C > 65535 ||
        chain0 < 0 || p <= 0 || !(sigma > 0.0)) {
        qn_set_error("%s: bad argument", who);
        return QN_EINVAL;
    }
    const double gs = -0.5 / (sigma * sigma);
    (void)hipGetLastError();
    with_flags<TE>(scale, beta, [&](auto hs, auto hb) {
        hipLaunchKernelGGL((k_hmc_begin<TE, decltype(hs)::value, decltype(hb)::value>), dim3(hmc_parts(p), C), dim3(HBLK), 0,
                           static_cast<hipStream_t>(stream), cur, grad_cur, eps, scale, beta, gs, chain0, p, seed, step_ptr,
                           mom, q, kin_cur_parts);
    });
    QN_HIP_CHECK(hipGetLastError());
    return QN_OK;
}

template <typename TE>
int hmc_leap_launch(const char* who, const void* grad_q, int dtype, double sigma, TE eps, const double* scale,
                    const double* beta, int last, int C, int64_t p, double* mom, double* q, double* kin_prop_parts,
                    void* stream) {
    if (!grad_q || eps_missing(eps) || !mom || !q || (last && !kin_prop_parts) || C <= 0 || C > 65535 || p <= 0 ||
        !(sigma > 0.0) || (dtype != QN_F64 && dtype != QN_F32)) {
        qn_set_error("%s: bad argument", who);
        return QN_EINVAL;
    }
    const double gs = -0.5 / (sigma * sigma);
    const double f = last ? 0.5 : 1.0;
    const int l = last ? 1 : 0;
    (void)hipGetLastError();
    with_flags<TE>(scale, beta, [&](auto hs, auto hb) {
        const dim3 grid(hmc_parts(p), C), blk(HBLK);
        hipStream_t st = static_cast<hipStream_t>(stream);
        if (dtype == QN_F32)
            hipLaunchKernelGGL((k_hmc_leap<float, TE, decltype(hs)::value, decltype(hb)::value>), grid, blk, 0, st,
                               (const float*)grad_q, eps, scale, beta, f, gs, l, p, mom, q, kin_prop_parts);
        else
            hipLaunchKernelGGL((k_hmc_leap<double, TE, decltype(hs)::value, decltype(hb)::value>), grid, blk, 0, st,
                               (const double*)grad_q, eps, scale, beta, f, gs, l, p, mom, q, kin_prop_parts);
    });
    QN_HIP_CHECK(hipGetLastError());
    return QN_OK;
}

}  // namespace

extern "C" int qn_hmc_begin(const double* cur, const double* grad_cur, double sigma, double epsilon, int C, int chain0,
                            int64_t p, uint64_t seed, const int64_t* step_ptr, double* mom, double* q, double* kin_cur_parts,
                            void* stream) {
    return hmc_begin_launch("qn_hmc_begin", cur, grad_cur, sigma, epsilon, nullptr, nullptr, C, chain0, p, seed, step_ptr, mom,
                            q, kin_cur_parts, stream);
}

extern "C" int qn_hmc_leap(const void* grad_q, int dtype, double sigma, double epsilon, int last, int C, int64_t p, double* mom,
                           double* q, double* kin_prop_parts, void* stream) {
    return hmc_leap_launch("qn_hmc_leap", grad_q, dtype, sigma, epsilon, nullptr, nullptr, last, C, p, mom, q, kin_prop_parts,
                           stream);
}

extern "C" int qn_hmc_begin_s(const double* cur, const double* grad_cur, double sigma, const double* eps,
                              const double* scale, int C, int chain0, int64_t p, uint64_t seed, const int64_t* step_ptr,
                              double* mom, double* q, double* kin_cur_parts, void* stream) {
    return hmc_begin_launch("qn_hmc_begin_s", cur, grad_cur, sigma, eps, scale, nullptr, C, chain0, p, seed, step_ptr, mom, q,
                            kin_cur_parts, stream);
}

extern "C" int qn_hmc_leap_s(const void* grad_q, int dtype, double sigma, const double* eps, const double* scale, int last,
                             int C, int64_t p, double* mom, double* q, double* kin_prop_parts, void* stream) {
    return hmc_leap_launch("qn_hmc_leap_s", grad_q, dtype, sigma, eps, scale, nullptr, last, C, p, mom, q, kin_prop_parts,
                           stream);
}

extern "C" int qn_hmc_begin_t(const double* cur, const double* grad_cur, double sigma, const double* eps, const double* scale,
                              const double* beta, int C, int chain0, int64_t p, uint64_t seed, const int64_t* step_ptr,
                              double* mom, double* q, double* kin_cur_parts, void* stream) {
    return hmc_begin_launch("qn_hmc_begin_t", cur, grad_cur, sigma, eps, scale, beta, C, chain0, p, seed, step_ptr, mom, q,
                            kin_cur_parts, stream);
}

extern "C" int qn_hmc_leap_t(const void* grad_q, int dtype, double sigma, const double* eps, const double* scale,
                             const double* beta, int last, int C, int64_t p, double* mom, double* q, double* kin_prop_parts,
                             void* stream) {
    return hmc_leap_launch("qn_hmc_leap_t", grad_q, dtype, sigma, eps, scale, beta, last, C, p, mom, q, kin_prop_parts,
                           stream);
}
