// tanh to ABSOLUTE accuracy 2^-51 on a table of tanh(n / 512): the activation of the 8-wave int8-slice forward
// (k_fused_fwd_i8<.., PAIR = true>, qn_fused_i8.hip), which has the LDS for the 80 KB table.  Part of qn_math.h; kept in a
// file of its own, free of device-only calls, so that a host program can compile the very same arithmetic
// (tests/test_tanh_tab512_cpu.py compares it with an extended-precision reference at every node, every midpoint and
// random points).
//   |x| = n / 512 + b, |b| <= 2^-10 exact (min, fma with 512 and 1.5 2^52, subtract, fma: as qn_tanh_f64_tab64)
//   tb = b - b^3 / 3                                   dropped: (2/15) b^5 <= 2^-52.9
//   tanh = T + (1 - T^2) tb (1 - e)(1 + e^2), e = T tb dropped: tb e^4 (1 - T^2) <= 2^-50 max T^4 (1 - T^2) = 2^-52.7
// 14 float64 instructions with the sign copy (qn_tanh_f64_tab64: 16), still one 8-byte table read per element.
#pragma once
#include "qn_tanh_table512.h"
#include <cmath>
#include <cstdint>
#include <cstring>
#if defined(__HIPCC__)
#define QN_TANH512_FN __host__ __device__ __forceinline__
#else
#define QN_TANH512_FN inline
#endif

QN_TANH512_FN double qn_tanh_f64_tab512(double x, const double* __restrict__ tab) {
    const double kMagic = 6755399441055744.0;                          // 1.5 * 2^52
#if defined(__HIP_DEVICE_COMPILE__)
    double ax;
    asm("v_min_f64 %0, |%1|, %2" : "=v"(ax) : "v"(x), "s"(20.0));
    const double zm = fma(ax, 512.0, kMagic);                          // 512|x| rounded to an integer n in 0..10240
    const int n = __double2loint(zm);
#else
    const double ax = std::fmin(std::fabs(x), 20.0);
    const double zm = std::fma(ax, 512.0, kMagic);
    std::uint64_t bits;
    std::memcpy(&bits, &zm, 8);
    const int n = (int)(std::uint32_t)bits;
    using std::fma;
#endif
    const double T = tab[n];                                           // tanh(n / 512)
    const double b = fma(zm - kMagic, -0.001953125, ax);               // exact, |b| <= 2^-10
    const double b2 = b * b;
    const double tb = fma(b * b2, -3.33333333333333333e-01, b);
    const double e = T * tb;
    const double w = fma(-tb, e, tb);                                  // tb (1 - e)
    const double u = fma(w, e * e, w);                                 // tb (1 - e)(1 + e^2)
    return __builtin_copysign(fma(fma(-T, T, 1.0), u, T), x);
}
