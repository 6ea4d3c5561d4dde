// Device helpers shared by the sampler translation units (qn_mcmc.hip, qn_hmc_leap.hip, qn_hmc_adapt.hip, qn_temper.hip, qn_sgmcmc.hip, qn_prior.hip, qn_hyper.hip, qn_noise.hip, qn_ess.hip, qn_nuts.hip): the Philox4x32-10 generator and
// its counter layout, the normal / uniform transforms, the 8-byte aligned pair accesses and the geometry + fixed-order block
// sum of the HMC elementwise kernels.  Everything is internal linkage: each translation unit gets its own copy.
#pragma once
#include "qn_common.h"
#include <cmath>

namespace {

struct Philox {
    uint32_t c[4], k[2];
    __device__ __forceinline__ void round() {
        const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u;
        const uint32_t hi0 = __umulhi(M0, c[0]), lo0 = M0 * c[0];
        const uint32_t hi1 = __umulhi(M1, c[2]), lo1 = M1 * c[2];
        const uint32_t n0 = hi1 ^ c[1] ^ k[0], n1 = lo1, n2 = hi0 ^ c[3] ^ k[1], n3 = lo0;
        c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
        k[0] += 0x9E3779B9u; k[1] += 0xBB67AE85u;
    }
    // 4 x 32 random bits for (seed, stream, counter)
    __device__ __forceinline__ void gen(uint64_t seed, uint64_t stream, uint64_t ctr) {
        c[0] = (uint32_t)ctr; c[1] = (uint32_t)(ctr >> 32); c[2] = (uint32_t)stream; c[3] = (uint32_t)(stream >> 32);
        k[0] = (uint32_t)seed; k[1] = (uint32_t)(seed >> 32);
#pragma unroll
        for (int r = 0; r < 10; ++r) round();
    }
};

// Philox counter of one draw: [global chain id : 24][purpose : 4][index : 36].  The chain id is GLOBAL
// (chain0 + local index), so a chain's random numbers do not depend on how chains are split over launches /
// ranks.  purposes: 0 elementwise normals (index = column pair), 1 per-chain scalar normal, 2 accept uniform,
// 3 history coefficients (index = row pair); 4 minibatch rows and 5 step noise (qn_sgmcmc.hip); 6 the exchange uniform
// (qn_temper.hip); 7 the ellipse partner (index = column pair) and 8 the angle uniforms (index = shrink count) of elliptical
// slice sampling (qn_ess.hip); 9 the momenta (index = column pair) and 10 the scalar uniforms (index = (kind << 32) | n: kind 0
// the direction of doubling n, 1 the merge of doubling n, 2 the leaf whose n_leap was n) of the No-U-Turn sampler
// (qn_nuts.hip); 11 the Gamma variates of the hyper-prior's Gibbs round (qn_hyper.hip; stream 2 t + 1, index =
// (group << 16) | (attempt << 4) | block); 12 the Gamma variate of the noise level's Gibbs round (qn_noise.hip; stream
// 2 t + 1, index = (attempt << 4) | block).  13-15 are free
__device__ __forceinline__ uint64_t ctr_of(int chain, int purpose, uint64_t index) {
    return ((uint64_t)chain << 40) | ((uint64_t)purpose << 36) | (index & 0xFFFFFFFFFull);
}

// uniform in (0, 1) with 53 random bits
__device__ __forceinline__ double u01(uint32_t hi, uint32_t lo) {
    const uint64_t bits = ((uint64_t)hi << 21) ^ (uint64_t)(lo >> 11);        // 53 bits
    return ((double)bits + 0.5) * (1.0 / 9007199254740992.0);
}

// two independent standard normals (Box-Muller) from one Philox block.  Proposal noise does not need float64
// transcendental functions (they made the propose / apply kernels compute-bound, ~9 us per step at cfg2): the
// radius and the angle are formed with the hardware float32 log2 / sin / cos (angle in revolutions), ~1e-6
// relative accuracy, tails to 8 sigma; the accept test keeps its 53-bit uniform.
__device__ __forceinline__ void normal2(const Philox& ph, double& a, double& b) {
    const uint32_t hi = ph.c[0] >> 8;                                                     // 24 bits
    // (0, 1); the lowest of the 2^24 bins is subdivided by 24 more bits so that the tails reach 8 sigma
    const float u1t = hi ? ((float)hi + 0.5f) * (1.0f / 16777216.0f)
                         : ((float)(ph.c[1] >> 8) + 0.5f) * (1.0f / 16777216.0f) * (1.0f / 16777216.0f);
    const float u2 = (float)(ph.c[2] >> 8) * (1.0f / 16777216.0f);                        // [0, 1) revolutions
    const float r = __builtin_sqrtf(-1.3862943611198906f * __builtin_amdgcn_logf(u1t));   // sqrt(-2 ln u1), ln = ln2 * log2
    a = (double)(r * __builtin_amdgcn_cosf(u2));
    b = (double)(r * __builtin_amdgcn_sinf(u2));
}

typedef double d2u __attribute__((ext_vector_type(2), aligned(8)));      // two doubles at an 8-byte aligned address
typedef float f2u __attribute__((ext_vector_type(2), aligned(4)));
__device__ __forceinline__ d2u ld2(const double* p, bool both) {
    if (both) return *reinterpret_cast<const d2u*>(p);
    d2u v; v.x = p[0]; v.y = 0.0; return v;                          // (the last element of an odd-length row)
}
__device__ __forceinline__ void st2(double* p, double x, double y, bool both) {
    if (both) { d2u v; v.x = x; v.y = y; *reinterpret_cast<d2u*>(p) = v; } else p[0] = x;
}

// ---- Hamiltonian Monte Carlo on the device (quinn/mcmc/hmc.py:43-66 around the batched gradient kernel).
// Elementwise over [C, p], HBM-bound: begin 2 reads + 2 writes, leap 3 reads + 2 writes of 8 B per element.  A
// chain's elements are spread over HPARTS(p) workgroups of HBLK threads x HUB elements; each writes ONE partial sum
// of squares (fixed-order tree inside the block), the accept kernel adds the partials left to right: kinetic energies
// are bitwise reproducible and depend only on p, never on how many chains a launch or a rank holds.
constexpr int HBLK = 256;
constexpr int HUB = 4;
__device__ __forceinline__ double block_sum_256(double v, double* red) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}
inline int hmc_parts(int64_t p) {                      // workgroups per chain: a function of p alone (see k_hmc_begin, qn_hmc_leap.hip)
    const int64_t n = (p + HBLK * HUB - 1) / (HBLK * HUB);
    return n > 64 ? 64 : (n < 1 ? 1 : (int)n);
}

}  // namespace
