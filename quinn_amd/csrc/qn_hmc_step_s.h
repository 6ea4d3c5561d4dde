// The leapfrog kernels with a per-chain step size and a diagonal mass (qn_hmc_begin_s / qn_hmc_leap_s, qn_hmc_adapt.hip) and,
// with HB, a per-chain inverse temperature beta [C] (qn_hmc_begin_t / qn_hmc_leap_t, qn_temper.hip): the force is
// beta_c * d logpost, formed as gs_c = gs * beta_c, which then stands wherever the untempered kernel uses gs; drifts are
// unchanged.  HB is a compile-time choice: the HB = false instantiations are the untempered kernels, instruction for
// instruction, and a tempered call with beta = 1 gives their results bit for bit (gs * 1 == gs).
#pragma once
#include "qn_mcmc_shared.h"

namespace {

// mom = z + (hk_c s) g_cur;  q = cur + (eps_c s) mom;  K_cur partial = sum z^2       (hk_c = (eps_c / 2) gs, gs = -0.5 / sigma^2)
// One Philox block = one PAIR of consecutive elements = one 16-byte access per array (8-byte aligned: rows of odd length).
template <bool HB>
__global__ __launch_bounds__(HBLK) void k_hmc_begin_s(const double* __restrict__ cur, const double* __restrict__ gcur,
                                                      const double* __restrict__ eps, const double* __restrict__ scale,
                                                      const double* __restrict__ beta, double gs, int chain0, int64_t p,
                                                      uint64_t seed, const int64_t* __restrict__ step_ptr,
                                                      double* __restrict__ mom, double* __restrict__ q,
                                                      double* __restrict__ kin_parts) {
    __shared__ double red[4];
    const int b = blockIdx.y;
    const uint64_t step = (uint64_t)*step_ptr;
    const double eps_c = eps[b];
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
        const d2u sv = scale ? ld2(scale + base + e, both) : one;
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

// mom += (kick_c s) g;   last ? K_prop partial = sum mom^2 : q += (eps_c s) mom        (kick_c = f eps_c gs, f = 1 or 1/2)
// The element -> thread map and the order of the sum of squares are k_hmc_leap's.  HS: a scale array is given (a compile-time
// choice, so that the unrolled loads carry no per-element branch).
template <typename TG, bool HS, bool HB>
__global__ __launch_bounds__(HBLK) void k_hmc_leap_s(const TG* __restrict__ g, const double* __restrict__ eps,
                                                     const double* __restrict__ scale, const double* __restrict__ beta,
                                                     double f, double gs, int last, int64_t p, double* __restrict__ mom,
                                                     double* __restrict__ q, double* __restrict__ kin_parts) {
    __shared__ double red[4];
    const int b = blockIdx.y;
    const double eps_c = eps[b];
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

// The launches behind qn_hmc_begin_s / qn_hmc_begin_t and qn_hmc_leap_s / qn_hmc_leap_t (arguments already checked).
inline void hmc_begin_s_launch(const double* cur, const double* grad_cur, double sigma, const double* eps, const double* scale,
                               const double* beta, int C, int chain0, int64_t p, uint64_t seed, const int64_t* step_ptr,
                               double* mom, double* q, double* kin_cur_parts, hipStream_t st) {
    const double gs = -0.5 / (sigma * sigma);
    const dim3 grid(hmc_parts(p), C), blk(HBLK);
    if (beta)
        hipLaunchKernelGGL(k_hmc_begin_s<true>, grid, blk, 0, st, cur, grad_cur, eps, scale, beta, gs, chain0, p, seed, step_ptr,
                           mom, q, kin_cur_parts);
    else
        hipLaunchKernelGGL(k_hmc_begin_s<false>, grid, blk, 0, st, cur, grad_cur, eps, scale, beta, gs, chain0, p, seed, step_ptr,
                           mom, q, kin_cur_parts);
}
template <typename TG, bool HB>
inline void hmc_leap_s_launch1(const void* grad_q, const double* eps, const double* scale, const double* beta, double f, double gs,
                               int l, int C, int64_t p, double* mom, double* q, double* kin_prop_parts, hipStream_t st) {
    const dim3 grid(hmc_parts(p), C), blk(HBLK);
    if (scale)
        hipLaunchKernelGGL((k_hmc_leap_s<TG, true, HB>), grid, blk, 0, st, (const TG*)grad_q, eps, scale, beta, f, gs, l, p, mom, q,
                           kin_prop_parts);
    else
        hipLaunchKernelGGL((k_hmc_leap_s<TG, false, HB>), grid, blk, 0, st, (const TG*)grad_q, eps, scale, beta, f, gs, l, p, mom, q,
                           kin_prop_parts);
}
inline void hmc_leap_s_launch(const void* grad_q, int dtype, double sigma, const double* eps, const double* scale,
                              const double* beta, int last, int C, int64_t p, double* mom, double* q, double* kin_prop_parts,
                              hipStream_t st) {
    const double gs = -0.5 / (sigma * sigma);
    const double f = last ? 0.5 : 1.0;
    const int l = last ? 1 : 0;
    if (dtype == QN_F32 && beta) hmc_leap_s_launch1<float, true>(grad_q, eps, scale, beta, f, gs, l, C, p, mom, q, kin_prop_parts, st);
    else if (dtype == QN_F32) hmc_leap_s_launch1<float, false>(grad_q, eps, scale, beta, f, gs, l, C, p, mom, q, kin_prop_parts, st);
    else if (beta) hmc_leap_s_launch1<double, true>(grad_q, eps, scale, beta, f, gs, l, C, p, mom, q, kin_prop_parts, st);
    else hmc_leap_s_launch1<double, false>(grad_q, eps, scale, beta, f, gs, l, C, p, mom, q, kin_prop_parts, st);
}

}  // namespace
